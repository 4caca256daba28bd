"""deepsense6g_tii_amd: the DeepSense-6G fusion models on hand-written gfx950 kernels (libds6g.so).

The submodules are imported by name (``deepsense6g_tii_amd.model``, ``.mamba_fuser``, ``.train`` ...).  The frozen inference
engine of MambaFuser is also exported here, resolved on first use so that importing the package stays free of side effects:

    from deepsense6g_tii_amd import MambaFuserEngine, freeze
"""

_LAZY = {"MambaFuserEngine": "mamba_infer", "freeze": "mamba_infer"}
__all__ = sorted(_LAZY)


def __getattr__(name):
    if name in _LAZY:
        from importlib import import_module
        return getattr(import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
