"""
The autoregressive spline head (csrc/arspline.hip) and the layer built on it (layers.AutoregressiveSpline) restated in torch ops,
dtype-generic: masked ``F.linear`` -> (B, D, 3K - 1) raw parameters -> the spline of tests/_rqs.py.  The yard-stick in float64, its float32
twin on the same inputs, and (on device tensors) the model tests' layer-by-layer reference.

    weight ((3K - 1) D, H), bias ((3K - 1) D, ): row p D + d is parameter p of feature d;  mask (D, H) of 0 / 1: row d serves feature d
"""
import torch
import torch.nn.functional as F

from tests import _rqs as R


def head_params(a, weight, bias, mask, K):
    """the materialised conditioner output (B, (3K - 1) D) in the p D + d order"""
    return F.linear(a, weight * mask.repeat(3 * K - 1, 1), bias)


def head_raw(a, weight, bias, mask, K):
    """per-element raw parameters (B, D, 3K - 1)"""
    return R.from_channels(head_params(a, weight, bias, mask, K), mask.shape[0])


def head(a, weight, bias, mask, z, ld, K, bound, inverse=False, col=None):
    """(y, ld'): every feature (col None), or the one column ``col`` with every other column as in z"""
    y, l = R.rqs(z, head_raw(a, weight, bias, mask, K), K, bound, inverse=inverse)
    if col is None:
        return y, ld + l.sum(1)
    out = z.clone()
    out[:, col] = y[:, col]
    return out, ld + l[:, col]


def trunk(layer, zp):
    """the activated last hidden layer of the PERMUTED input"""
    h = zp
    for i in range(layer.num_hidden):
        h = torch.relu(F.linear(h, layer.weights[i] * layer.masks[i], layer.biases[i]))
    return h


def layer_forward_permuted(layer, zp, ld):
    """trunk + head on the permuted input (the map whose Jacobian is lower triangular)"""
    return head(trunk(layer, zp), layer.head_weight, layer.head_bias, layer.head_mask, zp, ld, layer.bins, layer.tail_bound)


def layer_forward(layer, z, ld):
    return layer_forward_permuted(layer, torch.mm(z, layer.perm), ld)


def layer_inverse(layer, y, ld):
    """D passes: pass i takes column i alone from the inverse under the conditioner of the columns recovered so far"""
    x = y.clone()
    for i in range(layer.in_out_chs):
        x, ld = head(trunk(layer, x), layer.head_weight, layer.head_bias, layer.head_mask, x, ld, layer.bins, layer.tail_bound, inverse=True, col=i)
    return torch.mm(x, layer.perm.t()), ld
