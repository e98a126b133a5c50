"""hamer.utils of the reference exports ``eval_pose`` and ``Evaluator`` (hamer/utils/__init__.py).  They resolve lazily here:
importing this package imports nothing else and does not load the HIP library."""

__all__ = ["eval_pose", "Evaluator"]


def __getattr__(name):
    if name in __all__:
        from . import pose_utils
        return getattr(pose_utils, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
