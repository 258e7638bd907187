"""HIP drop-in plugins for the records-backed hot path.

``hip_default()`` is the packaging the reference uses for backends: a profile function
returning plugin instances (waveform_analysis/core/plugins/profiles.py:20-62); register them
with ``ctx.register(p, allow_override=True)`` to replace the CPU plugins of the same name.
``hip_with_records()`` adds the records / wave_pool builders (raw files -> bundle on the GPU);
``hip_from_raw_files()`` adds st_waveforms built from the raw files on the GPU as well;
``hip_full()`` adds the tabular and event stages (df, df_events, df_paired) on top, the counterpart of the
reference's ``cpu_default()``.
"""

from .basic_features import HipBasicFeaturesPlugin
from .dataframe import HipDataFramePlugin
from .event_analysis import HipGroupedEventsPlugin, HipPairedEventsPlugin
from .filtered_waveforms import HipFilteredWaveformsPlugin
from .hit_finder import HipHitFinderPlugin
from .hit_grouped import HipHitGroupedPlugin
from .hit_merge import HipHitMergeClustersPlugin, HipHitMergedComponentsPlugin, HipHitMergePlugin
from .records import HipRecordsPlugin, HipWavePoolPlugin
from .s1_s2 import HipS1S2ClassifierPlugin
from .signal_peaks import HipSignalPeaksStreamPlugin
from .threshold_hit import HipThresholdHitPlugin
from .wave_pool_filtered import HipWavePoolFilteredPlugin
from .waveform_width import HipWaveformWidthPlugin
from .waveforms import HipWaveformsPlugin
from .width_integral import HipWaveformWidthIntegralPlugin


def hip_default():
    return [HipWavePoolFilteredPlugin(), HipThresholdHitPlugin(), HipBasicFeaturesPlugin(),
            HipWaveformWidthIntegralPlugin(), HipHitGroupedPlugin(), HipHitFinderPlugin(),
            HipFilteredWaveformsPlugin(), HipWaveformWidthPlugin(), HipS1S2ClassifierPlugin(),
            HipHitMergeClustersPlugin(), HipHitMergePlugin(), HipHitMergedComponentsPlugin(),
            HipSignalPeaksStreamPlugin()]


def hip_with_records():
    """hip_default() plus records / wave_pool built from raw_files on the GPU (the pool then stays resident for the
    records-route plugins of the same thread)."""
    return hip_default() + [HipRecordsPlugin(), HipWavePoolPlugin()]


def hip_from_raw_files():
    """hip_with_records() plus st_waveforms built from raw_files on the GPU (the root of the dense chain
    st_waveforms -> filtered_waveforms -> hit -> waveform_width -> s1_s2)."""
    return hip_with_records() + [HipWaveformsPlugin()]


def hip_full():
    """hip_from_raw_files() plus df, df_events (grouped on the GPU) and df_paired: every product of the reference's
    cpu_default() profile (io + waveform + peaks + basic_features + tabular + events)."""
    return hip_from_raw_files() + [HipDataFramePlugin(), HipGroupedEventsPlugin(), HipPairedEventsPlugin()]


def hip_streaming():
    """The chunk streams: hit_threshold_stream, signal_peaks_stream and s1_s2_stream -- the counterpart of the
    reference's placeholder streaming_default() (profiles.py: "not available yet").  Register them beside a profile
    that provides records / wave_pool (and st_waveforms / filtered_waveforms for signal_peaks_stream)."""
    from ..s1s2_stream import HipS1S2Stream  # (these modules import the plugins package)
    from ..streaming import HipThresholdHitStream

    return [HipThresholdHitStream(), HipSignalPeaksStreamPlugin(), HipS1S2Stream()]


def hip_streaming_events():
    """hip_streaming() plus hit_grouped_stream: the coincidence events of the records stream, delivered as they close."""
    from ..event_stream import HipHitGroupedStream

    return hip_streaming() + [HipHitGroupedStream()]


def hip_streaming_merged():
    """hip_streaming_events() plus hit_merged_stream: the per-channel merged hits of the records stream, delivered as
    their clusters close."""
    from ..merge_stream import HipHitMergedStream

    return hip_streaming_events() + [HipHitMergedStream()]


def hip_streaming_merged_events():
    """hip_streaming_merged() plus hit_merged_grouped_stream: the coincidence events of the merged hits, delivered as
    they close -- the streamed form of hit_grouped whenever merging is on."""
    from ..merged_event_stream import HipHitMergedGroupedStream

    return hip_streaming_merged() + [HipHitMergedGroupedStream()]


def hip_streaming_df_events():
    """hip_streaming() plus basic_features_stream and df_events_stream: the features and the fixed-window coincidence
    events of the default chain (basic_features -> df -> df_events), delivered as the events close."""
    from ..df_event_stream import HipGroupedEventsStream
    from ..features_stream import HipBasicFeaturesStream

    return hip_streaming() + [HipBasicFeaturesStream(), HipGroupedEventsStream()]


def hip_streaming_records():
    """hip_streaming() plus records_stream: records and wave_pool from V1725 files, block by block -- the head of the
    chain; hit_threshold_stream takes its chunks (files -> hits in bounded memory)."""
    from ..records_stream import HipRecordsStream

    return hip_streaming() + [HipRecordsStream()]


__all__ = ["hip_streaming", "hip_streaming_records", "hip_streaming_events", "hip_streaming_df_events", "hip_streaming_merged", "hip_streaming_merged_events", "HipWavePoolFilteredPlugin", "HipThresholdHitPlugin", "HipBasicFeaturesPlugin",
           "HipWaveformWidthIntegralPlugin", "HipHitGroupedPlugin", "HipHitFinderPlugin", "HipFilteredWaveformsPlugin",
           "HipWaveformWidthPlugin", "HipS1S2ClassifierPlugin", "HipHitMergeClustersPlugin",
           "HipHitMergePlugin", "HipHitMergedComponentsPlugin", "HipSignalPeaksStreamPlugin", "HipRecordsPlugin", "HipWavePoolPlugin",
           "HipWaveformsPlugin", "HipDataFramePlugin", "HipGroupedEventsPlugin", "HipPairedEventsPlugin", "hip_default",
           "hip_with_records", "hip_from_raw_files", "hip_full"]
