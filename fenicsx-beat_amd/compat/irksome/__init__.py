"""``irksome``: the Butcher tableaux a reference script passes to ``beat.irksome_model.IrksomeMonodomainModel``
(tests/test_irksome_monodomain.py, demos/irksome_model_gotranx.py), from beat.butcher.  Irksome's form language and
steppers are not provided: the model does its own stepping."""

from beat.butcher import (  # noqa: F401
    Alexander,
    BackwardEuler,
    ButcherTableau,
    GaussLegendre,
    LobattoIIIA,
    LobattoIIIC,
    RadauIIA,
)

__all__ = ["Alexander", "BackwardEuler", "ButcherTableau", "GaussLegendre", "LobattoIIIA", "LobattoIIIC", "RadauIIA"]
