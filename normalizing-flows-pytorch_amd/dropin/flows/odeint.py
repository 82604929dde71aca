"""flows.odeint: the reference's own module from the user's checkout by default (see flows/__init__.py); with NF_DROPIN_FFJORD=1
``odeint`` / ``odeint_adjoint`` on the engine's ODENet: the whole integration in one launch, the adjoint gradient in two."""
import sys

from . import FFJORD_ENGINE, _pkg, reference_module

if FFJORD_ENGINE:
    odeint, odeint_adjoint = _pkg.odeint, _pkg.odeint_adjoint
    SOLVERS = dict(_pkg.functional.CNF_METHODS)
else:
    sys.modules[__name__] = reference_module('odeint')
