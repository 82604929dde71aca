"""flows.ffjord: the reference's own module from the user's checkout by default (see flows/__init__.py); with NF_DROPIN_FFJORD=1 the
engine's Ffjord (whole-integration HIP kernels, csrc/cnf.hip) under the reference's names."""
import sys

from . import FFJORD_ENGINE, _pkg, reference_module

if FFJORD_ENGINE:
    Ffjord, CNF, ActNorm, Compose = _pkg.Ffjord, _pkg.CNF, _pkg.ActNorm, _pkg.Compose
else:
    sys.modules[__name__] = reference_module('ffjord')
