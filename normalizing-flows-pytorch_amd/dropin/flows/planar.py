"""flows.planar: the reference's own module from the user's checkout by default (see flows/__init__.py); with NF_DROPIN_PLANAR=1 the
engine's PlanarFlow / PlanarTransform (HIP kernels) under the reference's names."""
import sys

from . import PLANAR_ENGINE, _pkg, reference_module

if PLANAR_ENGINE:
    PlanarFlow, PlanarTransform, Compose, BatchNorm = _pkg.PlanarFlow, _pkg.PlanarTransform, _pkg.Compose, _pkg.BatchNorm
else:
    sys.modules[__name__] = reference_module('planar')
