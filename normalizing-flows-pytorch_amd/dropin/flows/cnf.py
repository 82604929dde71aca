"""flows.cnf: the reference's own module from the user's checkout by default (see flows/__init__.py); with NF_DROPIN_FFJORD=1 the
engine's CNF / ODENet / ConcatLinear (parameter holders of the integration kernels) under the reference's names."""
import sys

from . import FFJORD_ENGINE, _pkg, reference_module

if FFJORD_ENGINE:
    CNF, ODENet, ConcatLinear = _pkg.CNF, _pkg.ODENet, _pkg.ConcatLinear
    odeint, odeint_adjoint = _pkg.odeint, _pkg.odeint_adjoint
else:
    sys.modules[__name__] = reference_module('cnf')
