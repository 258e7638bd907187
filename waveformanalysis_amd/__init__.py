"""ROCm-native waveform analysis: HIP kernels behind the reference's plugin and accessor interfaces."""

__all__ = ["HipRecordsView", "hip_records_view"]


def __getattr__(name):
    if name in __all__:  # resolved on first use: importing the package stays free of ctypes / numpy work
        from . import records_view

        return getattr(records_view, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
