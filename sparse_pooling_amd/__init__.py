"""SHPL on MI355X. Submodules are imported by name; ``FusionConcatBN`` (fusion_bn.py) is also reachable from
the package, loaded on first use."""


def __getattr__(name):
    if name == "FusionConcatBN":
        from .fusion_bn import FusionConcatBN
        return FusionConcatBN
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
