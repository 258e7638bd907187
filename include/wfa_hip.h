/*
 * wfa_hip.h -- C ABI of libwfa_hip.so, the MI355X (gfx950) backend for the per-record
 * waveform hot path of SnowingWolf/WaveformAnalysis.
 *
 * The reference is pure Python; there is no FFI to replace.  Each entry point below names
 * the reference function whose inner loop it replaces (paths relative to
 * waveform_analysis/).  The Python plugins in waveformanalysis_amd/plugins/ bind these
 * through ctypes (waveformanalysis_amd/_lib.py); INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - plain C, caller-allocated host buffers, no callbacks;
 *   - every function returns 0 on success or a negative WFA_E_* code;
 *     wfa_last_error() returns the message of the calling thread's last failure;
 *   - one wfa_ctx per (GPU, host thread); a ctx owns one HIP stream (plus a second one that
 *     only wfa_upload_dense_rows uses, idle again when it returns) and its device
 *     buffers; calls on one ctx are serialised by the caller;
 *   - the pool and the records SoA stay resident in HBM between calls, so
 *     filter -> hits -> features read them without another host transfer.
 */
#ifndef WFA_HIP_H
#define WFA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WFA_ABI_VERSION 12

#define WFA_OK 0
#define WFA_E_INVALID (-1)   /* bad argument / malformed records (maps to ValueError) */
#define WFA_E_HIP (-2)       /* HIP runtime failure */
#define WFA_E_STATE (-3)     /* call order: something required was not uploaded / planned */
#define WFA_E_NOMEM (-4)
#define WFA_E_RCCL (-5)
#define WFA_E_LIMIT (-6)     /* record longer than WFA_MAX_RECORD_SAMPLES etc. */

/* The plain threshold kernel keeps a record's hit bitmap in LDS (one 64-bit word per 64 samples, 4 waves per block,
 * 64 KiB): 2038 words.  The streaming hit kernel (k_sg_runs32) packs a run edge as (record << 16) | sample and is only
 * chosen for uniform records of at most 65 504 samples; longer uniform records take the bitmap route.  Everything else
 * indexes samples with 32-bit integers and sums them in 64 bits. */
#define WFA_MAX_RECORD_SAMPLES 130432
#define WFA_MAX_SG_WINDOW 63
/* wfa_sosfiltfilt: second-order sections per filter (a Butterworth band-pass of order N has N sections) */
#define WFA_MAX_SOS_SECTIONS 32
/* wfa_hits_enqueue_groups: filter groups of one grouped hit pass, and resident plan slots (wfa_sg_plan_store) */
#define WFA_MAX_HIT_GROUPS 8

/* wave source of a consumer (reference: cpu/_wave_source.py:119-165, records branch) */
#define WFA_SRC_RAW 0        /* wave_pool (uint16)                                        */
#define WFA_SRC_F32 1        /* wave_pool_filtered (float32) resident on the device       */
#define WFA_SRC_SG_FUSED 2   /* Savitzky-Golay of wave_pool evaluated on the fly, never   */
                             /* materialised (the fused baseline+filter+hitfind pass)     */

/* polarity code per record (reference: records["polarity"], dtypes.py:87) */
#define WFA_POL_UNKNOWN 0
#define WFA_POL_NEGATIVE 1
#define WFA_POL_POSITIVE 2
/* dense st_waveforms rule of BasicFeaturesPlugin (basic_features.py:243-262): wave-based formulas, positive sign;
 * every other stage treats it like WFA_POL_UNKNOWN */
#define WFA_POL_POSITIVE_WAVE 3

typedef struct wfa_ctx wfa_ctx;

int wfa_abi_version(void);
int wfa_device_count(int* count);
int wfa_last_error(char* buf, size_t buf_len);

int wfa_ctx_create(int device_id, wfa_ctx** out);
void wfa_ctx_destroy(wfa_ctx* ctx);
int wfa_sync(wfa_ctx* ctx);
/* Free the device scratch a later call rebuilds by itself (hit bitmap, run-event buffer, padded shadow pool, candidate
 * and sort buffers, filter scratch, the samples of the last wfa_csv_decode_fill); the resident pools, the records, the
 * plan, the rows of the last passes and the CSV sample arena stay.
 * This is what Plugin.cleanup(context) of the HIP plugins calls (core/plugins/core/base.py:608-613: "releasing
 * resources" after compute()).  freed_bytes (nullable) receives the capacity given back. */
int wfa_release_scratch(wfa_ctx* ctx, int64_t* freed_bytes);
/* Capacity (bytes) of that same scratch as it stands: what wfa_release_scratch would give back now.  Read only; it
 * bounds the device memory a pass holds beyond its inputs and outputs (e.g. the hit-table slots of a grouping pass). */
int wfa_scratch_bytes(wfa_ctx* ctx, int64_t* bytes);
/* Choice between code paths that produce identical results (no counterpart in the reference: its plugins have one
 * code path).  For tests, which compare the paths with each other, and for measurement; a caller never needs it.
 * Names (any other name: WFA_E_INVALID):
 *   "no_fast"        literal float64 hit kernel instead of the integer kernels
 *   "no_span"        per-record mask kernel instead of the uniform-record kernels
 *   "no_pad"         no padded shadow layout
 *   "no_runs32"      bitmap route instead of the run-event (streaming) kernel
 *   "no_speculate"   exact row launches (host round trip for the hit count)
 *   "no_deposit"     streaming kernel: the flush reads the records' last samples from memory again
 *   "span_records"   streaming kernel: records per span (value; 0 = the library's choice)
 *   "no_peak_hot"    find_peaks: the plateau machine over every sample, no height prefilter
 *   "no_peak_slots"  find_peaks: count + fill walks instead of one walk into per-record slots */
int wfa_set_option(wfa_ctx* ctx, const char* name, int value);
/* GB/s of the last pool upload through the pinned staging ring (uploads of >= 4 MiB are copied chunk by chunk into two
 * pinned 32-MiB buffers while the previous chunk is on the wire; reference: the plugins hold host arrays only). */
int wfa_last_h2d_rate(wfa_ctx* ctx, double* gb_per_s);
/* Source of the device-resident THRESHOLD_HIT_DTYPE rows that wfa_hit_merge_count / wfa_group_hit_windows_count read
 * when ALL their column pointers are NULL: 1 = rows of the last hit pass (default), 2 = rows the last
 * wfa_rccl_gather_rows left on the root.  Replaces the host columns hit_merge.py:115-181 / event_grouping.py:418-471
 * take from the structured array: no upload, no download between the stages. */
int wfa_hit_rows_source(wfa_ctx* ctx, int which);

/* ---- resident inputs -------------------------------------------------------------------- */

/* wave_pool: flat uint16 samples (reference: processing/records_builder.py:197,299;
 * plugins/builtin/cpu/records.py:321-331). */
int wfa_upload_pool_u16(wfa_ctx* ctx, const uint16_t* pool, int64_t n_samples);

/* wave_pool_filtered produced elsewhere (reference: records.py:334-438 output).  With the same sample count as
 * the resident wave_pool it becomes its float32 twin; with a different count it replaces the pool set (the
 * uint16 pool is dropped and records must be uploaded again). */
int wfa_upload_pool_f32(wfa_ctx* ctx, const float* pool, int64_t n_samples);

/* The samples of a dense array (st_waveforms / filtered_waveforms) as the resident pool, unpacked ON THE DEVICE
 * (reference: cpu/_wave_source.py load_wave_input hands such an array to the dense branches hit_finder.py:179-255,
 * peak_finding.py:336-343 and basic_features.py:197-278, which read data["wave"] row by row).  `rows` = the memory of a
 * C-contiguous 1-D structured array: n_rows rows of row_bytes bytes, each with wave_length elements at byte wave_offset
 * (ST_WAVEFORM_DTYPE, processing/dtypes.py:18-64: wave at byte 76, rows of 76 + 2 L bytes).  elem:
 *   WFA_DENSE_I16  int16 samples read as uint16 ADC codes; a sample with the sign bit set is an error
 *   WFA_DENSE_U16  uint16 samples
 *   WFA_DENSE_F32  float32 samples, copied bit for bit (NaN payloads, -0.0, infinities)
 * Whole rows go through the pinned staging ring in batches of at most batch_bytes (at least one row, at most 1 GiB)
 * into two device buffers in turn; k_dense_unpack writes batch k into the pool in row-major order (sample j of row r at
 * r * wave_length + j) on a second stream while batch k + 1 is copied.  Afterwards the context is in the state
 * wfa_upload_pool_u16 (I16 / U16) or wfa_upload_pool_f32 (F32) of the n_rows * wave_length samples leaves.
 * WFA_E_INVALID before any launch: a negative count, wave_offset or row_bytes no multiple of the element size,
 * wave_offset + wave_length * itemsize > row_bytes.  n_rows == 0 or wave_length == 0: an empty pool, no launch.
 * I16 with a negative sample: WFA_E_INVALID, *first_negative_row (nullable; -1 otherwise) = the smallest row that holds
 * one, and the context is left without a pool and without records. */
#define WFA_DENSE_I16 0
#define WFA_DENSE_U16 1
#define WFA_DENSE_F32 2
int wfa_upload_dense_rows(wfa_ctx* ctx, const void* rows, int64_t n_rows, int64_t row_bytes, int32_t wave_offset,
                          int32_t wave_length, int elem, int64_t batch_bytes, int64_t* first_negative_row);

/* Records index table as structure-of-arrays (reference row layout: processing/dtypes.py:80-100;
 * the per-channel option lookups of hit_finder.py:288-327 are resolved by the caller into
 * `threshold`).  Validates 0 <= offset, 0 <= length <= WFA_MAX_RECORD_SAMPLES,
 * offset+length <= pool size (reference: data/records_view.py:47-56). */
int wfa_upload_records_soa(wfa_ctx* ctx, int64_t n_records,
                           const int64_t* wave_offset, const int32_t* event_length,
                           const double* baseline, const int8_t* polarity_code,
                           const double* threshold, const int64_t* timestamp,
                           const int32_t* dt_ns, const int16_t* board, const int16_t* channel,
                           const int64_t* record_id);

/* The same table as packed rows, unpacked ON THE DEVICE: `rows` = n_records rows of row_bytes bytes exactly as a numpy
 * structured array holds them (reference RECORDS_DTYPE, core/processing/dtypes.py:80-100: 102 bytes, unaligned).
 * field_offsets[9] = byte offset inside a row of wave_offset (int64), event_length (int32), baseline (float64), polarity
 * (UCS-4 text of polarity_chars characters: "negative" / "positive" / anything else = unknown, as
 * data/records_view.py:87-100 reads it), timestamp (int64), dt (int32), board (int16), channel (int16), record_id (int64);
 * -1 for an absent polarity / dt / board / channel (defaults unknown / 1 / 0 / 0).  `threshold` applies to every record
 * unless `thresholds` (nullable, one float64 per record: hit_finder.py:288-327 resolved by the caller) is given;
 * `polarity` (nullable, one WFA_POL_* code per record) overrides the text field.  Same validation and messages as the
 * column route.  *record_ids_increasing = 0 tells the caller that record_id is not strictly increasing (it then has to
 * check uniqueness itself: records_view.py:383-400); *max_len = longest record. */
int wfa_upload_records_packed(wfa_ctx* ctx, const void* rows, int64_t n_records, int32_t row_bytes,
                              const int32_t* field_offsets, int32_t polarity_chars, double threshold,
                              const double* thresholds, const int8_t* polarity, int32_t* max_len,
                              int* record_ids_increasing);

/* Savitzky-Golay plan (reference: cpu/filtering.py:181-195,226-240 + scipy.signal.savgol_filter
 * mode="interp").  Tables are built on the host (waveformanalysis_amd/sg_plan.py):
 *   n_tables = (window+1)/2; table t serves effective window w = 2t+1 (short records,
 *   filtering.py:187-193); a table with w <= polyorder is unused (filter is a copy).
 *   tab: n_tables * (window + 2*(window/2)*window) doubles:
 *        [ fw[window] | E_left[window/2][window] | E_right[window/2][window] ] per table
 *        fw = correlation weights (savgol_coeffs reversed), E = polynomial edge projection.
 *   symmetric[t]: the branch ndimage.correlate1d takes for fw: 1 symmetric, 2 anti-symmetric, 0 general.
 *   Integer plan for the full window (exact rational arithmetic):
 *        itab: [ n[window] | NL[window/2][window] | NR[window/2][window] ] int32,
 *        y = n.x / den (interior), edges N.x / den_edge; guard_* = |numerator| below which
 *        the kernel evaluates the float64 chain instead.  int_ok = 0 disables it. */
int wfa_set_sg_plan(wfa_ctx* ctx, int window, int polyorder, const double* tab,
                    const uint8_t* symmetric, int int_ok, const int32_t* itab, int32_t den,
                    int32_t den_edge, int64_t guard, int64_t guard_edge);

/* ---- kernels ---------------------------------------------------------------------------- */

/* K1 baseline estimate: mean of samples [start, min(end, event_length)) of every record as
 * float64, NaN when that range is empty (reference: records_builder.py:243-257,
 * waveforms.py:714-733).  start >= 0, or WFA_E_INVALID; both ends are clamped to the longest
 * uploaded record on the host, which changes no result (here and in the fused passes below).
 * Writes the device-resident baseline column when update_records != 0; out may be NULL. */
int wfa_baseline_mean(wfa_ctx* ctx, int32_t start, int32_t end, int update_records, double* out);

/* Filter channel groups with different settings into ONE wave_pool_filtered (reference: per-channel
 * filter configs of build_filter_batches, cpu/filtering.py:339-374).  keep = 0 (default): wfa_savgol /
 * wfa_sosfiltfilt zero the whole output first (gaps stay 0.0, records.py:382) and then write the uploaded
 * records' slices.  keep = 1: the output is left as it is and only the uploaded records' slices are written. */
int wfa_filter_keep_output(wfa_ctx* ctx, int keep);

/* Copy the resident float32 pool (wave_pool_filtered as built or uploaded) to the host; n_samples must match. */
int wfa_download_pool_f32(wfa_ctx* ctx, float* out, int64_t n_samples);

/* Copy samples [start, start + n) of the resident float32 pool to the host (one shard's part of a run's
 * wave_pool_filtered, or the samples of some of its records).  0 <= start, 0 <= n, start + n <= the pool's samples. */
int wfa_download_pool_f32_range(wfa_ctx* ctx, float* out, int64_t start, int64_t n);

/* K2 wave_pool_filtered: float32 pool aligned to wave_pool, gaps 0.0
 * (reference: records.py:368-438, filtering.py:377-407).  The result stays resident as the
 * WFA_SRC_F32 pool; out may be NULL. */
int wfa_savgol(wfa_ctx* ctx, float* out);

/* K3 wave_pool_filtered, Butterworth branch: scipy.signal.sosfiltfilt per record, float64 recursion,
 * float32 result (reference: filtering.py:84-101,198-224).  sos = n_sections x 6 coefficients from
 * scipy.signal.butter(..., output="sos"), zi = n_sections x 2 from scipy.signal.sosfilt_zi, padlen =
 * the reference's _estimate_sosfiltfilt_padlen; records with length <= padlen are copied.  The result
 * stays resident as the WFA_SRC_F32 pool; out may be NULL.  1 <= n_sections <= WFA_MAX_SOS_SECTIONS. */
int wfa_sosfiltfilt(wfa_ctx* ctx, int n_sections, const double* sos, const double* zi, int32_t padlen,
                    float* out);

/* K4 threshold hits (reference: hit_finder.py:231-255,329-413).  Two-phase so the caller can
 * allocate the structured array: _count runs the pass and returns the number of rows,
 * _fill copies them (THRESHOLD_HIT_DTYPE, 60-byte packed rows, order = record index, start).
 * max_len = padded matrix width of the reference call (max event_length over the whole
 * records array, hit_finder.py:364,370); pass 0 to use the maximum of the uploaded records. */
int wfa_threshold_hits_count(wfa_ctx* ctx, int source, int32_t left_extension,
                             int32_t right_extension, int32_t max_len, int64_t* n_hits);
int wfa_threshold_hits_fill(wfa_ctx* ctx, void* out_rows, int64_t n_hits);

/* K7 fused pass: baseline estimate over [bl_start, bl_end) (skipped if bl_end <= bl_start:
 * the uploaded baseline is used) + Savitzky-Golay + threshold hits in one read of the pool. */
int wfa_fused_baseline_filter_hits(wfa_ctx* ctx, int32_t bl_start, int32_t bl_end,
                                   int32_t left_extension, int32_t right_extension,
                                   int32_t max_len, int64_t* n_hits);

/* The same passes without a host round trip: _enqueue queues the whole pass on the context's stream and returns (the
 * row kernels are launched for the previous pass's row count + 12 % and read the real count on the device); _wait
 * blocks for the last enqueued pass and returns its row count, redoing the pass the exact way in the rare case that it
 * found more rows than that bound.  source = WFA_SRC_RAW / _F32 / _SG_FUSED; the baseline window applies to
 * WFA_SRC_SG_FUSED only (bl_end <= bl_start: uploaded baselines).  A context's first pass (no previous count) runs to
 * completion inside _enqueue.  wfa_threshold_hits_fill waits by itself.  (Streaming callers and bench.py use this
 * pair: consecutive chunks' passes run back to back on the device.) */
int wfa_hits_enqueue(wfa_ctx* ctx, int source, int32_t bl_start, int32_t bl_end, int32_t left_extension,
                     int32_t right_extension, int32_t max_len);
int wfa_hits_wait(wfa_ctx* ctx, int64_t* n_hits);

/* The grouped hit pass: hits of ONE uploaded records table whose channels resolve to several filter settings, merged on
 * the device into one table (reference: cpu/filtering.py:339-374 groups the records by their resolved settings;
 * hit_finder.py:288-327 resolves the per-channel threshold; hit_finder.py:354-366 emits the hits of all records in one
 * loop, i.e. by (record index, start)).  Streaming callers queue it: nobody waits for chunk k before chunk k + 1.
 *
 * wfa_sg_plan_store keeps a Savitzky-Golay plan in slot `slot` (0 <= slot < WFA_MAX_HIT_GROUPS), arguments as for
 * wfa_set_sg_plan.  A slot's tables stay on the device across pool and records uploads; wfa_set_sg_plan and the plan it
 * sets are untouched.
 *
 * wfa_sosfiltfilt_group is wfa_sosfiltfilt restricted to the records r with group_of_record[r] == group (one int32 per
 * uploaded record), over the uploaded table: the records are not uploaded again, so the padded shadow and the layout
 * record stand.  It writes those records' slices of the float32 twin and nothing else (a twin that did not exist is
 * zeroed first), downloads nothing and does not wait for the device.
 *
 * wfa_savgol_group is its Savitzky-Golay twin: wfa_savgol under the plan kept in `slot` (wfa_sg_plan_store), restricted
 * to the records r with group_of_record[r] == group, over the uploaded table.  It writes those records' slices of the
 * float32 twin and nothing else (a twin that did not exist is zeroed first), downloads nothing, does not wait for the
 * device and waits out a pending queued hit pass first; the plan of wfa_set_sg_plan is untouched.  The route is the one
 * wfa_savgol takes for the uploaded table (k_savgol_span on uniform records, padded or not, k_savgol on ragged ones); a
 * record that is not a member is neither loaded nor stored.  The written samples are byte-identical to wfa_savgol on
 * a table that holds only the member records, records shorter than the window included.  So a chunk whose channels
 * resolve to several filter settings gets its float32 twin from one call per setting, with the whole chunk's table
 * resident for the stages behind (wfa_find_peaks_count, wfa_peak_chain_count).
 * WFA_E_INVALID: slot out of range, group_of_record NULL with records uploaded.  WFA_E_STATE: no records or no
 * wave_pool uploaded, a slot without a stored plan.
 *
 * wfa_hits_enqueue_groups queues, on the context's stream, the table of n_groups passes over the uploaded records.
 * The table: group g (in order) contributes the rows of one hit pass under the plan of groups[g].plan_slot
 * (WFA_SRC_SG_FUSED) or from the float32 twin (WFA_SRC_F32), in which only the records with group_of_record[r] == g can
 * hit: every other record's threshold reads +inf during that pass (sig >= +inf holds for no finite sample: no hit on any
 * route).  group_of_record[r] = -1: no pass owns record r, it gives no rows.  Baselines: [bl_start, bl_end) as in
 * wfa_hits_enqueue -- the WFA_SRC_SG_FUSED groups estimate the baselines over that window inside their pass (and leave
 * them on the device), bl_end <= bl_start means the uploaded baselines; WFA_SRC_F32 groups always read the baselines as
 * they stand.
 * Merge order: ascending record index; the rows of one record keep the order of the pass that produced them (by start),
 * and rows of one record that came from two passes would stand in group order -- group_of_record gives a record to one
 * group, so that does not occur.  The table is byte-identical to the host merge of the groups' single passes.
 * How it is queued: the masked column of a group is written by a kernel from group_of_record, the plan is chosen by
 * slot, the rows of a pass go to a stash under a row count read on the device (launches sized for the pass's bound), the
 * stash offsets are written on the device and the merge kernels (k_hit_rows_merge_*: per-record row count, exclusive
 * scan, scatter of the 60-byte rows as 15 dwords each) take their totals from there.
 * Speculation and redo: where every group's pass takes the speculative row launch (a warm context: each group's
 * previous row count is kept, per group index; uniform records on the streaming or bitmap route) the call returns with
 * nothing waited for and wfa_hits_wait delivers the merged count; if a group found more rows than its bound, or a span's
 * events overflowed, wfa_hits_wait redoes the grouped pass the exact way.  A group whose pass cannot speculate (the
 * general route on ragged records, a context's first grouped pass, no_speculate) runs to completion inside the call, as
 * in wfa_hits_enqueue.  n_groups == 1 without a -1 runs the single pass: no mask kernel, no stash, no merge.
 * Afterwards the merged table IS "the rows of the last hit pass": wfa_threshold_hits_fill, wfa_hits_wait,
 * wfa_rccl_gather_rows(rows = NULL) and, through wfa_hit_rows_source(ctx, 1), the resident hit-table stages read it; its
 * row count sizes the next single pass's speculative launch; and the uploaded threshold column reads as the caller
 * uploaded it.
 * The stash is scratch (wfa_release_scratch frees it, wfa_scratch_bytes counts it): 64 bytes per stashed row + 8 per
 * merged row, beside the table itself.
 * WFA_E_INVALID: n_groups outside [1, WFA_MAX_HIT_GROUPS], a source other than the two above, a plan slot or a
 * group_of_record value out of range, bl_start < 0 with bl_end > bl_start, max_len below the longest uploaded record
 * (0 = that record).  WFA_E_STATE: no records or no wave_pool uploaded, a slot without a stored plan, a WFA_SRC_F32
 * group without a resident float32 pool (wfa_sosfiltfilt_group / wfa_upload_pool_f32 first).
 *
 * wfa_hits_pending: *pending = 1 from a queued pass (wfa_hits_enqueue / _groups) until wfa_hits_wait or
 * wfa_threshold_hits_fill has consumed it, else 0.  Reads state only. */
typedef struct wfa_hit_group {
    int32_t source;    /* WFA_SRC_SG_FUSED or WFA_SRC_F32 */
    int32_t plan_slot; /* WFA_SRC_SG_FUSED: the slot of wfa_sg_plan_store; ignored for WFA_SRC_F32 */
} wfa_hit_group;
int wfa_sg_plan_store(wfa_ctx* ctx, int slot, int window, int polyorder, const double* tab, const uint8_t* symmetric,
                      int int_ok, const int32_t* itab, int32_t den, int32_t den_edge, int64_t guard, int64_t guard_edge);
int wfa_sosfiltfilt_group(wfa_ctx* ctx, int n_sections, const double* sos, const double* zi, int32_t padlen,
                          const int32_t* group_of_record, int32_t group);
int wfa_savgol_group(wfa_ctx* ctx, int slot, const int32_t* group_of_record, int32_t group);
int wfa_hits_enqueue_groups(wfa_ctx* ctx, int n_groups, const wfa_hit_group* groups, const int32_t* group_of_record,
                            int32_t bl_start, int32_t bl_end, int32_t left_extension, int32_t right_extension,
                            int32_t max_len);
int wfa_hits_pending(wfa_ctx* ctx, int* pending);

/* K8 find_peaks-based hit detector, records source (reference: cpu/peak_finding.py:395-614 calling
 * scipy.signal.find_peaks(det, height, distance, prominence, width, threshold) with scalar lower bounds, then
 * _calculate_peak_height 567-614).  source: WFA_SRC_RAW or WFA_SRC_F32.  Two-phase like the threshold hits; rows
 * are HIT_DTYPE (48 B packed: position i8, height f4, integral f4, edge_start f4, edge_end f4, dt i4,
 * timestamp i8, board i2, channel i2, record_id i8) in (record, position) order.  has_threshold = 0 means
 * threshold=None.  An empty minmax window fails with numpy's "zero-size array ..." message (WFA_E_INVALID). */
#define WFA_HEIGHT_MINMAX 0
#define WFA_HEIGHT_DIFF 1
/* signal_mode: WFA_PEAK_SIGNAL_RECORDS = records branch (signal = -rv.signals(id): float32 (w - baseline), sign by
 * polarity; detection on diff(signal) or signal).  WFA_PEAK_SIGNAL_ROWS = dense st_waveforms / filtered_waveforms
 * branch (peak_finding.py:316-378): the stored samples are the waveform, pulses are negative-going (detection on
 * -diff(row) in the row's dtype or float64 baseline - row), the height is measured on the row itself. */
#define WFA_PEAK_SIGNAL_RECORDS 0
#define WFA_PEAK_SIGNAL_ROWS 1
/* WFA_PEAK_SIGNAL_ROWS_F64 = the streaming detector (streaming/cpu/signal_peaks.py:226-406): like _ROWS, but the row
 * is converted to float64 first (detection on -diff in float64), rows are never cut at event_length, and the 'diff'
 * height is cumsum(-diff(row))[end] - cumsum[start] with numpy's sequential cumsum, rounded to float32. */
#define WFA_PEAK_SIGNAL_ROWS_F64 2
int wfa_find_peaks_count(wfa_ctx* ctx, int source, int signal_mode, int use_derivative, double height, int has_threshold,
                         double threshold, int32_t distance, double prominence, double width, int height_method,
                         int32_t height_window_extension, int64_t* n_peaks);
int wfa_find_peaks_fill(wfa_ctx* ctx, void* out_rows, int64_t n_peaks);

/* K5 basic features (reference: basic_features.py:108-195).  Ranges are python slice bounds;
 * *_has_end = 0 means "None".  fixed_baseline: per-record override, NaN = none, may be NULL.
 * out: BASIC_FEATURES_DTYPE rows (36 B). */
int wfa_basic_features(wfa_ctx* ctx, int source, int64_t height_start, int64_t height_end,
                       int height_has_end, int64_t area_start, int64_t area_end, int area_has_end,
                       const double* fixed_baseline, void* out_rows);

/* K14 legacy threshold crossings on dense rows (reference: processing/event_grouping.py:46-95 `find_hits`):
 * mask = (baselines[row] - wave) > threshold in float64, one hit per 0 -> 1 transition.  The resident pool is the
 * row-major wave matrix (as for K10).  fill: event_index / start sample of every hit in row-major order. */
int wfa_find_hits_count(wfa_ctx* ctx, int source, int64_t n_rows, int32_t row_length, const double* baselines,
                        double threshold, int64_t* n_hits);
int wfa_find_hits_fill(wfa_ctx* ctx, int64_t n_hits, int64_t* event_index, int64_t* start_sample);

/* K10 rise/fall/total width per hit on dense waveform rows (reference: cpu/waveform_width.py:205-374).
 * The resident pool is the row-major (n_rows x row_length) wave matrix of st_waveforms (source WFA_SRC_RAW,
 * non-negative int16 ADC codes viewed as uint16) or filtered_waveforms (WFA_SRC_F32).  Per hit: position and
 * the row it refers to (row_index < 0: no such row, hit skipped).  out: WAVEFORM_WIDTH_DTYPE rows (56 B) with the
 * six width fields, peak_position and peak_height filled, the id fields zero (the caller copies them from the
 * hit table); valid[i] = 0 where the reference drops the hit (position past the row, peak value <= 0).
 * Arithmetic follows numpy's promotion rules for the source dtype (float64 for int16 rows, float32 for
 * float32 rows incl. its mixed python-float cases), so the float fields are bit-exact. */
int wfa_waveform_width(wfa_ctx* ctx, int source, int64_t n_hits, const int64_t* position,
                       const int64_t* row_index, int64_t n_rows, int32_t row_length, double rise_low,
                       double rise_high, double fall_high, double fall_low, double sampling_rate,
                       int interpolation, void* out_rows, uint8_t* valid);

/* K10 on the resident records: the same rows without a dense matrix (reference: cpu/waveform_width.py:205-374,
 * `_calculate_width_from_peak` applied to waveform = pool[wave_offset[r] : wave_offset[r] + event_length[r]]).
 * record_index[i] = r is an INDEX into the uploaded records table (as the `hit` records branch fetches its waveform,
 * peak_finding.py:401-407), position[i] = p the sample inside that record.  valid[i] = 0 (hit dropped) when r is
 * outside [0, n_records), p >= event_length[r] (so every hit of an empty record), p < 0, or the peak value is <= 0.
 * The baseline is mean(first min(50, event_length[r]) samples of the record).  source: WFA_SRC_RAW (wave_pool, uint16:
 * float64 arithmetic) or WFA_SRC_F32 (wave_pool_filtered: float32 arithmetic with numpy 2's weak-scalar rules); pulses
 * are positive-going in stored counts, as in the reference.  Needs uploaded records and that source's pool
 * (WFA_E_STATE otherwise); everything else as wfa_waveform_width, bit-exact float fields included. */
int wfa_waveform_width_records(wfa_ctx* ctx, int source, int64_t n_hits, const int64_t* position,
                               const int64_t* record_index, double rise_low, double rise_high, double fall_high,
                               double fall_low, double sampling_rate, int interpolation, void* out_rows,
                               uint8_t* valid);

/* Peak chain: the S1/S2 rows of the resident find_peaks rows without a table leaving the device (reference: the chain
 * hit -> waveform_width -> s1_s2 with basic_features on the side: cpu/waveform_width.py:205-374,
 * cpu/basic_features.py:108-195, cpu/s1_s2_classifier.py:57-69,133-228).  Two-phase like the other row stages.
 * Needs uploaded records, the pool(s) of the two sources, and a wfa_find_peaks_count pass in signal mode
 * WFA_PEAK_SIGNAL_RECORDS whose rows are still resident (WFA_E_STATE otherwise).  count, on the context's stream:
 *  1. basic_features of the uploaded records (feature_source, height / area ranges as for wfa_basic_features; no
 *     fixed baseline in wfa_peak_chain_count, the column `fixed_baseline` in wfa_peak_chain_count_fixed) into a buffer
 *     of the stage -- the leaf kernel where wfa_basic_features would take it;
 *  2. k_peak_chain, one lane per peak row: the width of wfa_waveform_width_records (width_source) at (record_id,
 *     position) of the row, record_id being the INDEX of the record and of its feature row; a peak that call would mark
 *     valid = 0 is dropped.  Range cuts on float64(width), float64(area), float64(height): class_ranges = 6 x (lo, hi)
 *     in the order s1 width, s1 area, s1 height, s2 width, s2 area, s2 height; bit 2k / 2k + 1 of range_bounds says
 *     range k has a lower / an upper bound (the other reads as None), neither bit: the range is disabled.  NaN is outside
 *     every enabled range, a class with no enabled range never matches.  width_in_samples != 0 cuts on
 *     total_width_samples instead of total_width.  Both classes match: conflict_policy decides;
 *  3. scan of the keep flags, k_peak_chain_compact: the kept rows in peak order.
 * Rows are S1_S2_CLASSIFIER_DTYPE (45 B packed: label i1, width_ns f4, width_samples f4, height f4, area f4,
 * timestamp i8, board i2, channel i2, record_id i8, peak_position i8), bit-exact; record_id = the peak's record_id +
 * record_id_base (a chunk uploaded with chunk-local ids delivers the run's).  No peaks: 0 rows, nothing launched.
 * sampling_rate 0 / NaN: WFA_E_INVALID "float division by zero".  The peak rows (wfa_find_peaks_fill still delivers
 * them), pools, records and plan are untouched.  A records upload (or a pool upload, which drops the records) after
 * the find_peaks pass voids its rows for this stage: WFA_E_STATE until the pass has run on the new table.
 * Scratch (wfa_release_scratch frees it, wfa_scratch_bytes counts it; fill after a release: WFA_E_STATE):
 *   36 B per record + 45 B per peak + 45 B per kept row.
 * The keep flags and their scan reuse two per-candidate buffers of find_peaks, which that pass has finished with
 * once its rows exist; they cost 12 B per peak and 8 B per 1024 peaks + 8 B only where a release has taken them.
 *
 * wfa_peak_chain_count_fixed takes the arguments of wfa_peak_chain_count, then fixed_baseline (one float64 per uploaded
 * record, NaN = none: the override of wfa_basic_features, basic_features.py:143-146), then n_rows.  Step 1 is then
 * wfa_basic_features with that column: the feature rows in the stage's buffer equal that call's rows byte for byte.
 * The column is an argument of the call, not state of the context.  fixed_baseline = NULL is wfa_peak_chain_count
 * exactly, and wfa_peak_chain_count is that case of this entry. */
#define WFA_S1S2_UNKNOWN 0
#define WFA_S1S2_PREFER_S1 1
#define WFA_S1S2_PREFER_S2 2
int wfa_peak_chain_count(wfa_ctx* ctx, int width_source, int feature_source, double rise_low, double rise_high,
                         double fall_high, double fall_low, double sampling_rate, int interpolation,
                         int64_t height_start, int64_t height_end, int height_has_end, int64_t area_start,
                         int64_t area_end, int area_has_end, int width_in_samples, const double* class_ranges,
                         uint32_t range_bounds, int conflict_policy, int64_t record_id_base, int64_t* n_rows);
int wfa_peak_chain_count_fixed(wfa_ctx* ctx, int width_source, int feature_source, double rise_low, double rise_high,
                               double fall_high, double fall_low, double sampling_rate, int interpolation,
                               int64_t height_start, int64_t height_end, int height_has_end, int64_t area_start,
                               int64_t area_end, int area_has_end, int width_in_samples, const double* class_ranges,
                               uint32_t range_bounds, int conflict_policy, int64_t record_id_base,
                               const double* fixed_baseline, int64_t* n_rows);
int wfa_peak_chain_fill(wfa_ctx* ctx, void* out_rows, int64_t n_rows);

/* ---- hit-table stages (device sort + scans; host columns in, host index tables out) ----------------------
 * K11 hit merge (reference: cpu/hit_merge.py:115-181 `_build_merged_clusters`, 256-322 `_emit_cluster`).
 * Input: the columns of a hit table (THRESHOLD_HIT_DTYPE or its renamed variants).
 * count/fill = HitMergeClustersPlugin: per hardware channel (ascending board, channel) hits are ordered by
 * abs_start = ts + (edge_start - position) * dt * 1e3 (float64, stable) and chained while merge_gap_ns > 0, dt
 * unchanged, gap <= merge_gap and total width <= max_total_width.  fill: order[n] = hit index of each
 * cluster-ordered row (= hit_merge_clusters.hit_index) and cluster_offset[n_clusters + 1] into it.
 * emit = the per-cluster part of HitMergePlugin for ANY membership table (as the reference derives hit_merged
 * from whatever hit_merge_clusters holds): anchor hit index (max height, tie -> smallest timestamp, first such),
 * max height, sum of integrals (numpy's pairwise float64 order, as float32), min/max sample window (-1, -1 if the
 * cluster spans records) and width (-1 likewise). */
int wfa_hit_merge_count(wfa_ctx* ctx, int64_t n_hits, const int64_t* timestamp, const int64_t* position,
                        const int32_t* edge_start, const int32_t* edge_end, const int32_t* dt, const int16_t* board,
                        const int16_t* channel, double merge_gap_ns, double max_total_width_ns, int64_t* n_clusters);
int wfa_hit_merge_fill(wfa_ctx* ctx, int64_t n_hits, int64_t n_clusters, int64_t* order, int64_t* cluster_offset);
int wfa_hit_merge_emit(wfa_ctx* ctx, int64_t n_hits, const int64_t* timestamp, const int32_t* sample_start,
                       const int32_t* sample_end, const int64_t* record_id, const float* height, const float* integral,
                       int64_t n_members, const int64_t* member_hit, int64_t n_clusters, const int64_t* cluster_offset,
                       int64_t* anchor, float* out_height, float* out_integral, int32_t* out_start, int32_t* out_end,
                       float* out_width);

/* K9 event grouping (reference: processing/event_grouping.py:286-471 `group_hit_windows`).  Absolute windows as
 * above from (sample_start, sample_end); global order np.lexsort((record_id, timestamp, dt, abs_start)); a hit
 * opens a new event when abs_start > running max(abs_end) + time_window_ns * 1e3; inside an event hits are ordered
 * by (board, channel, dt, abs_start, timestamp, record_id).  abs_*_fix (both or neither, may be NULL): where not
 * NaN they replace the computed window (merged hits spanning records take the extent of their components,
 * event_grouping.py:371-416).  fill: order[n] (hit indices, event-major),
 * event_start[n_events + 1], t_min / t_max = int(min abs_start) / int(max abs_end) per event (ps). */
int wfa_group_hit_windows_count(wfa_ctx* ctx, int64_t n_hits, const int64_t* timestamp, const int64_t* position,
                                const int32_t* sample_start, const int32_t* sample_end, const int32_t* dt,
                                const int16_t* board, const int16_t* channel, const int64_t* record_id,
                                const double* abs_start_fix, const double* abs_end_fix, double time_window_ns,
                                int64_t* n_events);
int wfa_group_hit_windows_fill(wfa_ctx* ctx, int64_t n_hits, int64_t n_events, int64_t* order, int64_t* event_start,
                               int64_t* t_min, int64_t* t_max);

/* Event stream: K9 chunk by chunk, the hits of the events still open kept on the device between pushes.
 * A horizon H is a float64 such that every hit not yet pushed has computed abs_start >= H.  A push appends its
 * THRESHOLD_HIT_DTYPE rows (60 B, host memory; NULL with n_rows = 0 is a pure flush) behind the carried rows, runs the
 * grouping pass of wfa_group_hit_windows_count over that table (sample window = edge_start / edge_end) and closes
 * every event with max(abs_end) + time_window_ns * 1e3 < H, strictly: the closed events are a prefix of the table's
 * events, no later hit can join or precede them, and their ids continue the count of the events closed before.  The
 * hits of all other events stay on the device in their original row order (the carry) and are grouped again with the
 * next push's rows; after the last rows a push with H = +inf closes everything.  All rows pushed, in any chunking,
 * give the rows of the static pass over the whole table.
 * _push reports the rows and events this push closed and the rows carried; _fill delivers those rows, 84 B packed
 * (EVENT_HIT_DTYPE): event_id i8 @0, t_min i8 @8, t_max i8 @16 (truncated like the static pass), the hit's 60 bytes
 * unchanged @24; one row per hit, events in order, inside an event the static pass's order.
 * Refused with WFA_E_INVALID, the stream left as it was: a negative window (_begin); a pushed row with dt <= 0 or a
 * negative edge_start / edge_end; a pushed row whose abs_start lies below the previous push's horizon; a horizon
 * below the previous one, or NaN; carry + pushed rows >= 2^31.  _push without _begin, _fill before a push or after a
 * refused one: WFA_E_STATE; _fill with another row count: WFA_E_INVALID.  _begin on an open stream starts over.
 * The carry and the rows of the last push are state: wfa_release_scratch keeps them, wfa_scratch_bytes does not count
 * them, _end frees them (60 B per carried row in each of two buffers, 84 B per row of the largest push). */
int wfa_event_stream_begin(wfa_ctx* ctx, double time_window_ns);
int wfa_event_stream_push(wfa_ctx* ctx, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_out_rows,
                          int64_t* n_out_events, int64_t* n_carry);
int wfa_event_stream_fill(wfa_ctx* ctx, void* out_rows, int64_t n_out_rows);
int wfa_event_stream_end(wfa_ctx* ctx);

/* Merge stream: K11 chunk by chunk, the hits of the clusters still open kept on the device between pushes.
 * A horizon H is as for the event stream.  A push appends its THRESHOLD_HIT_DTYPE rows (60 B, host memory; NULL with
 * n_rows = 0 is a pure flush) behind the carried rows -- the carry keeps its original row order, so ties of the stable
 * sort fall where the whole table would put them -- and runs the sort and chain of wfa_hit_merge_count over that table.
 * In a channel's sorted table let F be the number of rows with abs_start < H, strictly.  A cluster at sorted positions
 * [a, b) is closed iff b <= F and one of: b < F (the hit that broke the chain is final); merge_gap_ns <= 0 (nothing ever
 * joins); H - cluster_end > merge_gap_ns * 1e3 in float64 (no later hit can join: its abs_start is >= H and float
 * subtraction is monotone).  Closed clusters are a prefix of every channel's clusters and final; the hits of all others
 * stay on the device (the carry) and are chained again with the next push's rows, which reproduces them because a chain
 * restarted at a cluster head gives the rest.  After the last rows a push with H = +inf closes everything.
 * _push reports the clusters closed, their members, the rows carried and open_start = the smallest abs_start among the
 * carried rows (+inf: none): below min(H, open_start) no merged row will start any more.  _fill delivers
 *   merged_rows: 72 B packed (HIT_MERGED_DTYPE), one per closed cluster, ordered by (board, channel), then chain order:
 *                the fields of wfa_hit_merge_emit's cluster on its anchor hit, a cluster of one hit being that hit;
 *                component_count as in the static table; component_offset = the offset of the cluster's members in the
 *                stream's own component sequence, cumulative over all pushes since _begin;
 *   hit_index:   one int64 per member, clusters in the order of the merged rows, members in chain order: the row's
 *                position in the sequence of all rows pushed since _begin.
 * Stably sorted by (board, channel), with component_offset rewritten as the running sum of component_count and the
 * members moved with their clusters, all pushes together give the static hit_merged, hit_merge_clusters.hit_index and
 * hit_merged_components of the whole table, in any chunking.
 * Refused with WFA_E_INVALID, the stream left as it was: a negative or NaN gap or width (_begin); a pushed row with
 * dt <= 0 or a negative edge_start / edge_end; a pushed row whose abs_start lies below the previous push's horizon; a
 * horizon below the previous one, or NaN; carry + pushed rows >= 2^31.  _push without _begin, _fill before a push or
 * after a refused one: WFA_E_STATE; _fill with other counts: WFA_E_INVALID.  _begin on an open stream starts over.  A
 * context may hold an open event stream and an open merge stream at once.
 * The carry and the output of the last push are state: wfa_release_scratch keeps them, wfa_scratch_bytes does not count
 * them, _end frees them (68 B per carried row in each of two buffers, 72 B per cluster and 8 B per member of the largest
 * push). */
int wfa_merge_stream_begin(wfa_ctx* ctx, double merge_gap_ns, double max_total_width_ns);
int wfa_merge_stream_push(wfa_ctx* ctx, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_merged,
                          int64_t* n_components, int64_t* n_carry, double* open_start_ps);
int wfa_merge_stream_fill(wfa_ctx* ctx, void* merged_rows, int64_t* hit_index, int64_t n_merged, int64_t n_components);
int wfa_merge_stream_end(wfa_ctx* ctx);

/* Merged-event stream: K9 over the rows of K11, chunk by chunk; the merged rows never visit the host.  One push
 * (THRESHOLD_HIT_DTYPE rows, H) does two steps on a state of its own (neither the event stream's nor the merge stream's;
 * all three may be open on one context):
 *  1. the merge step: the rule of wfa_merge_stream_push -- clusters close, the hits of the open ones stay in row order,
 *     open_start = the smallest computed abs_start still carried;
 *  2. the group step: the merged rows of the clusters just closed go behind the event carry, in the merge step's delivery
 *     order ((board, channel), then chain order), and the grouping pass of wfa_group_hit_windows_count runs over carry ++
 *     new rows.  A merged row with sample_start >= 0 and sample_end >= 0 takes the anchor formula; any other (its cluster
 *     spans records) takes min abs_start / max abs_end of its member hits, computed when the cluster closes and carried
 *     with the row (the abs_start_fix / abs_end_fix of the static pass).  An event closes iff
 *     max(abs_end) + time_window_ns * 1e3 < G, strictly, under the grouping horizon
 *         G = max(G of the previous push, min(H, open_start'))
 *     with open_start' = open_start where horizon_margin_ps == 0 and nextafter(open_start - 1.5 * horizon_margin_ps, -inf)
 *     otherwise: every merged row still to come starts at a carried hit or at a hit not yet pushed.  horizon_margin_ps is
 *     the run's margin as event_stream.horizon_margin gives it (2 ulp of the run's magnitude beyond 2^53 ps, else 0); the
 *     bound is 3 ulp because a computed member window and a computed anchor window each lie within 1.5 ulp of the exact
 *     start.  Below 2^53 ps min(H, open_start) never falls and the outer max changes nothing.
 *     Precondition: the hits of one record share timestamp - position * dt * 1e3 (threshold hits do), so that the anchor
 *     window of a one-record cluster starts where its first member does.  A violation is refused, never a wrong table.
 * All pushes together give the static K9 on the static K11 rows of the whole table (components included), in any chunking.
 * _push reports: rows and events the group step closed; clusters and members the merge step closed; hits carried by the
 * merge step and merged rows carried by the group step; G.  _fill delivers
 *   out_rows:  96 B packed (EVENT_MERGED_HIT_DTYPE): event_id i8 @0, t_min i8 @8, t_max i8 @16, then the 72 bytes of the
 *              HIT_MERGED_DTYPE row @24, component_offset counting through the stream's own component sequence;
 *   hit_index: one int64 per member of the clusters the MERGE step closed in this push (not: of the rows delivered), in
 *              the merge stream's order; concatenated over all pushes it is the sequence component_offset addresses.
 * Refused with WFA_E_INVALID, both carries and all counters left as they were: a negative or NaN gap, width or window, a
 * negative, NaN or infinite margin (_begin); a pushed row with dt <= 0 or a negative edge_start / edge_end (merged rows
 * with -1, -1 are legitimate inside); a pushed row below the previous push's H; a merged row below the previous push's G;
 * an H below the previous one, or NaN; either table reaching 2^31 rows.  _push without _begin, _fill before a push or
 * after a refused one: WFA_E_STATE; _fill with other counts: WFA_E_INVALID.  _begin on an open stream starts over.
 * State, not scratch: 68 B per carried hit and 88 B per carried merged row in each of two buffers, 96 B per row and 8 B
 * per member of the largest push; wfa_release_scratch keeps them, _end frees them. */
int wfa_merged_event_stream_begin(wfa_ctx* ctx, double merge_gap_ns, double max_total_width_ns, double time_window_ns,
                                  double horizon_margin_ps);
int wfa_merged_event_stream_push(wfa_ctx* ctx, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_out_rows,
                                 int64_t* n_out_events, int64_t* n_clusters, int64_t* n_components, int64_t* n_merge_carry,
                                 int64_t* n_event_carry, double* group_horizon_ps);
int wfa_merged_event_stream_fill(wfa_ctx* ctx, void* out_rows, int64_t* hit_index, int64_t n_out_rows, int64_t n_components);
int wfa_merged_event_stream_end(wfa_ctx* ctx);

/* Legacy fixed-window grouping: group_multi_channel_hits (processing/event_grouping.py:98-283) with the boundary search of
 * _find_cluster_boundaries_numba (475-525).  The hits are ordered by timestamp (stable; pandas' default sort leaves the
 * order of equal timestamps unspecified), a cluster takes every hit whose timestamp is <= (double)first + time_window_ps
 * (float64 comparison, as numpy / numba compare an int64 column with a float64 needle), and inside a cluster the hits
 * stand by channel (stable).  order[k] = input row of output row k (event-major); bounds[e] .. bounds[e + 1] = the rows of
 * event e in `order`.  time_window_ps = time_window_ns * 1e3, formed by the caller as the reference forms it. */
int wfa_group_multi_channel_count(wfa_ctx* ctx, int64_t n_hits, const int64_t* timestamp, const int64_t* channel,
                                  double time_window_ps, int64_t* n_events);
int wfa_group_multi_channel_fill(wfa_ctx* ctx, int64_t n_hits, int64_t n_events, int64_t* order, int64_t* bounds);

/* df_events stream: the fixed-window grouping above chunk by chunk, the rows of the events still open kept on the device
 * between pushes.  Input rows are 40 B (DF_ROW_DTYPE, host memory): timestamp i8 @0, record_id i8 @8, area f4 @16,
 * height f4 @20, amp f4 @24, max_abs_diff f4 @28, board i2 @32, channel i2 @34, reserved u4 @36 (must be 0).
 * A horizon H is an int64 such that every row not yet pushed has timestamp >= H.  A push appends its rows (NULL with
 * n_rows = 0 is a pure flush) behind the carried rows -- the carry keeps its original row order, so ties of the stable
 * sort fall where the whole table would put them -- and runs the sort and chain of wfa_group_multi_channel_count over
 * that table.  An event with anchor (first row's) timestamp a is closed iff (double)H > (double)a + time_window_ps,
 * strictly, in float64, or if the push is final (final != 0).  Anchors do not decrease and the conversion int64 ->
 * float64 is monotone: the closed events are a prefix of the chain, and a later row has
 * (double)ts >= (double)H > (double)a + time_window_ps >= (double) of every member, so it can neither join nor precede
 * them.  The rows of all other events stay on the device in row order (the carry) and are chained again with the next
 * push's rows.  All rows pushed, in any chunking, give the rows of the static pass over the whole table.
 * _push reports the rows and events this push closed and the rows carried; _fill delivers those rows, 64 B
 * (DF_EVENT_ROW_DTYPE): event_id i8 @0 (continuing the count of the events closed before), t_min i8 @8, t_max i8 @16 (the
 * timestamps of the event's first and last row after the channel sort, as the static pass: not the extremes),
 * timestamp i8 @24, record_id i8 @32, area f4 @40, height f4 @44, amp f4 @48, max_abs_diff f4 @52, n_hits i4 @56,
 * board i2 @60, channel i2 @62; one row per member, events in chain order, inside an event the static pass's order.
 * time_window_ps = time_window_ns * 1e3, formed by the caller as for the static pass.
 * Host waits of a push: one for the counts (the control block), as in wfa_event_stream_push, and, because the static
 * pass's radix sort is reused as it is, one per sort for its key ranges (two sorts: the table by timestamp, the closed
 * prefix by (event, channel)), one when the push ends, and one more in a push that has to grow the carry buffer; _fill
 * waits for its copy.
 * Refused with WFA_E_INVALID, the stream left as it was: a negative or NaN window (_begin); a pushed row whose timestamp
 * lies below the previous push's horizon; a horizon below the previous one; a pushed row with reserved != 0; carry +
 * pushed rows >= 2^31.  _push without _begin, _fill before a push or after a refused one: WFA_E_STATE; _fill with another
 * row count: WFA_E_INVALID.  _begin on an open stream starts over.  A context may hold this stream open beside the event,
 * merge and merged-event streams.
 * The carry and the rows of the last push are state: wfa_release_scratch keeps them, wfa_scratch_bytes does not count
 * them, _end frees them (40 B per carried row in each of two buffers, 64 B per row of the largest push). */
int wfa_df_event_stream_begin(wfa_ctx* ctx, double time_window_ps);
int wfa_df_event_stream_push(wfa_ctx* ctx, const void* rows, int64_t n_rows, int64_t horizon_ts, int final,
                             int64_t* n_out_rows, int64_t* n_out_events, int64_t* n_carry);
int wfa_df_event_stream_fill(wfa_ctx* ctx, void* out_rows, int64_t n_out_rows);
int wfa_df_event_stream_end(wfa_ctx* ctx);

/* ---- records builder (reference: processing/records_builder.py) -------------------------------------------------
 * K12 global record order: np.lexsort((seq, channel, board, pid, timestamp)) (records_builder.py:115-120), i.e. the
 * order a k-way merge of sorted parts produces (341-426, 869-945).  order[k] = source row of output row k. */
int wfa_records_sort(wfa_ctx* ctx, int64_t n_records, const int64_t* timestamp, const int32_t* pid,
                     const int16_t* board, const int16_t* channel, int64_t* order);

/* K13 pack the wave slices of the records, given in OUTPUT order, into one contiguous pool
 * (records_builder.py:195-207, 400-409).  src_pool: the concatenated source samples (uint16 bit patterns);
 * out_offset[r] receives the running sum of max(length, 0).  The packed pool becomes the resident wave_pool of the
 * context (records must be uploaded again); out_pool, when not NULL, also receives it.  src_pool = NULL with
 * src_samples > 0 takes the samples the last wfa_csv_decode_fill left on the device. */
int wfa_pool_gather(wfa_ctx* ctx, int64_t n_records, const int64_t* src_offset, const int32_t* length,
                    const uint16_t* src_pool, int64_t src_samples, int64_t* out_offset, uint16_t* out_pool,
                    int64_t out_samples);

/* K16 st_waveforms rows: n rows of numpy's packed create_record_dtype(wave_length) layout (reference:
 * processing/dtypes.py:36-64 ST_WAVEFORM_DTYPE; filled by core/plugins/builtin/cpu/waveforms.py:640-734
 * `WaveformStruct._structure_waveform`, :384-450 the streaming structurizer, :233-290 `_convert_v1725_to_st_waveforms`).
 * Row stride 76 + 2 * wave_length bytes: baseline f64 @0, baseline_upstream f64 @8, polarity 8 x UCS-4 @16,
 * timestamp i64 @48, record_id i64 @56, dt i32 @64, event_length i32 @68, board i16 @72, channel i16 @74,
 * wave i16[wave_length] @76 = the first min(src_len[r], wave_length) samples of the row's source slice, zeros after.
 * The samples come from `source`: WFA_ST_SRC_HOST = src_pool (src_samples samples, uploaded through the staging
 * ring), _CSV = the samples of the last wfa_csv_decode_fill, _ARENA = the CSV arena (src_samples = its filled
 * extent), _POOL = the resident wave_pool (e.g. left by wfa_pool_gather).  polarity[r] indexes polarity_table:
 * n_polarity (1..8) strings of 8 UCS-4 code points each, zero padded.  Rows are built on the device in batches of at
 * most batch_bytes (>= one row, <= 1 GiB) in two buffers, each batch copied into `out` (n x stride bytes, caller
 * owned) through the pinned staging ring while the next one is packed.  Slices and codes are checked before any
 * launch (WFA_E_INVALID). */
#define WFA_ST_SRC_HOST 0
#define WFA_ST_SRC_CSV 1
#define WFA_ST_SRC_ARENA 2
#define WFA_ST_SRC_POOL 3
int wfa_st_pack(wfa_ctx* ctx, int64_t n, int source, const uint16_t* src_pool, int64_t src_samples,
                const int64_t* src_offset, const int32_t* src_len, int32_t wave_length, const double* baseline,
                const double* baseline_upstream, const int64_t* timestamp, const int64_t* record_id, const int32_t* dt,
                const int32_t* event_length, const int16_t* board, const int16_t* channel, const uint8_t* polarity,
                const uint32_t* polarity_table, int32_t n_polarity, int64_t batch_bytes, uint8_t* out);

/* K17 padded waves / signals matrix of a list of records (reference: core/data/records_view.py:216-330
 * `RecordsView._waves_many` / `_signals_many`, one slice + cast + subtraction + two row assignments per record there).
 * Row r shows record rec_index[r] of the resident records table (0 <= rec_index[r] < n_records), L = its length:
 * end = min(sample_end < 0 ? L : sample_end, L), start = min(max(sample_start, 0), end); columns [0, end - start) hold
 * the transformed samples pool[offset + start ...], columns up to pad_len hold +0 (all bits zero), and mask (n_rows x
 * pad_len bytes, 0 / 1, may be NULL) marks the first.  Rows are pad_len * itemsize bytes, C order, no row padding.
 * source: WFA_SRC_RAW (resident uint16 pool) or WFA_SRC_F32 (resident float32 pool).
 * mode: _WAVES = cast only; _WAVES_BASELINE = x - b; _SIGNALS = x - b with the sign bit flipped iff the record's
 * polarity code is WFA_POL_POSITIVE (-0.0 where x == b, as numpy's unary minus gives).  b = baseline_override[r] when
 * baseline_override is not NULL (n_rows values), else the record's baseline.
 * out_dtype: _U16 (a copy; WFA_SRC_RAW in _WAVES mode only), _F32: float(x) - (float)b with b rounded to float once
 * (round to nearest even); _F64: (double)x - b.  One IEEE operation per sample.
 * rec_index outside the table, pad_len below a row's window length, negative n_rows / pad_len or another
 * mode / source / dtype combination: WFA_E_INVALID before any launch.  A request whose every window is empty (or
 * pad_len == 0) fills out / mask with zeros without a launch.  The matrix is built on the device in batches of at most
 * batch_bytes (>= one row, <= 1 GiB) in two buffers, each batch copied into out / mask (caller owned) through the
 * pinned staging ring while the next one is built. */
#define WFA_VIEW_WAVES 0
#define WFA_VIEW_WAVES_BASELINE 1
#define WFA_VIEW_SIGNALS 2
#define WFA_VIEW_U16 0
#define WFA_VIEW_F32 1
#define WFA_VIEW_F64 2
int wfa_view_gather(wfa_ctx* ctx, int64_t n_rows, const int64_t* rec_index, int32_t sample_start, int32_t sample_end,
                    int32_t pad_len, int mode, int source, int out_dtype, const double* baseline_override,
                    int64_t batch_bytes, void* out, uint8_t* mask);

/* K15 CAEN VX2730 CSV text -> integers on the device (reference: utils/formats/vx2730.py:78-110 column layout,
 * :193-340 `VX2730Reader.read_file` -- its polars / pyarrow / pandas backends all yield these integers; consumer
 * processing/records_builder.py:212-302).  text = the bytes of one or more files after their header rows: rows end
 * with '\n' (a '\r' before it is dropped, a last row without '\n' counts), fields are separated by `delimiter`.
 * _count uploads the text, indexes the rows and counts their fields; n_rows includes empty rows (0 fields).
 * n_samples = sum over rows of max(n_fields - samples_start, 0).
 * _fill parses columns meta_cols[0..n_meta) (each < samples_start) as int64 into meta[n_rows x n_meta] and the fields
 * from samples_start on as uint16 ADC codes into the ragged pool samples[sample_offset[r] ...]; row_offset[r] = byte
 * offset of row r in text (maps rows back to files), n_fields[r] = its field count.  Any output pointer but meta may
 * be NULL.  The samples stay resident: wfa_pool_gather with src_pool = NULL, src_samples = n_samples packs them
 * without a host round trip.  A requested field that is not a decimal integer, or a sample outside 0..65535, fails
 * with WFA_E_INVALID naming the row and field; other columns (ENERGY, FLAGS as hex, ...) are never parsed.
 * A decimal integer is [+-]?[0-9]{1,19} with a magnitude <= 2^63 - 1, and nothing else (no blanks, no empty field):
 *   - a field of 20 or more digits is refused even when its value is small (leading zeros count);
 *   - -9223372036854775808 is refused (the magnitude is tested before the sign is applied);
 *   - a meta column a row does not have reads 0; a column listed twice in meta_cols is filled twice.
 * Of several bad fields the one with the smallest (row, field) is named; "not a decimal integer" wins over the range
 * message for the same field.  After a failed _fill no decoded samples are resident. */
int wfa_csv_decode_count(wfa_ctx* ctx, const uint8_t* text, int64_t n_bytes, int delimiter, int32_t samples_start,
                         int64_t* n_rows, int64_t* n_samples);
int wfa_csv_decode_fill(wfa_ctx* ctx, int64_t n_rows, int32_t n_meta, const int32_t* meta_cols, int64_t* meta,
                        int64_t* row_offset, int32_t* n_fields, int64_t* sample_offset, uint16_t* samples,
                        int64_t n_samples);

/* K15 over a run of several parts (texts < 2^31 bytes each, cut after a '\n'): the decoded samples of every part go
 * to one context-owned sample arena, and one gather packs the run's wave_pool from it.
 * _reserve makes room for n_samples; keep_filled = 0 empties the arena (a new run), 1 keeps what is filled (growth).
 * _count is wfa_csv_decode_count with the text sent through the pinned staging ring.
 * _fill is wfa_csv_decode_fill writing part samples to arena[sample_base + sample_offset[r] ...]; sample_offset comes
 * back shifted by sample_base.  sample_base must lie in [0, filled] and sample_base + n_samples within the reserve
 * (checked before any launch); the filled extent grows to sample_base + n_samples.
 * _gather is wfa_pool_gather with the arena's filled extent as the source pool.
 * _filled reports the filled extent and the capacity (samples).  wfa_release_scratch keeps the arena. */
int wfa_csv_arena_reserve(wfa_ctx* ctx, int64_t n_samples, int keep_filled);
int wfa_csv_arena_count(wfa_ctx* ctx, const uint8_t* text, int64_t n_bytes, int delimiter, int32_t samples_start,
                        int64_t* n_rows, int64_t* n_samples);
int wfa_csv_arena_fill(wfa_ctx* ctx, int64_t sample_base, int64_t n_rows, int32_t n_meta, const int32_t* meta_cols,
                       int64_t* meta, int64_t* row_offset, int32_t* n_fields, int64_t* sample_offset, int64_t n_samples);
int wfa_csv_arena_gather(wfa_ctx* ctx, int64_t n_records, const int64_t* src_offset, const int32_t* length,
                         int64_t* out_offset, uint16_t* out_pool, int64_t out_samples);
int wfa_csv_arena_filled(wfa_ctx* ctx, int64_t* filled, int64_t* capacity);

/* Wave index of a CAEN V1725 DAW_DEMO binary stream held in host memory (reference: utils/formats/v1725.py:66-114
 * `V1725Reader.iter_waves`): 16-byte event header (channel mask in bytes 4 and 11), per set channel a 12-byte
 * header (size in 32-bit words: 22 bits, truncation flag bit 6 of byte 3, 48-bit timestamp bytes 4-9, uint16 baseline
 * bytes 10-11) + int16 payload.  Host-only, no context.  Call with capacity 0 to count, then with arrays of n_waves
 * entries.  payload_offset is in bytes from buf; a short header or payload ends the stream like the reference's reader. */
int wfa_v1725_index(const uint8_t* buf, int64_t n_bytes, int64_t capacity, int16_t* channel, int64_t* timestamp,
                    uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset, int32_t* n_samples, int64_t* n_waves);
/* The same walk over a window of a file (the same loop: one header decode).  at_file_end != 0: buf ends where the file
 * ends; wfa_v1725_index's result, *consumed_bytes = n_bytes.  at_file_end == 0: more of the file follows buf; only whole
 * events are indexed (n_waves counts their waves, no wave of an event that buf cuts), *consumed_bytes = where the last
 * whole event ends -- the next window starts there -- and 0 when buf holds not even one whole event: the caller reads
 * more.  Rows of the columns behind n_waves are not meaningful.  A channel block of fewer than 3 words is refused
 * (WFA_E_INVALID) wherever the walk meets one. */
int wfa_v1725_index_block(const uint8_t* buf, int64_t n_bytes, int at_file_end, int64_t capacity, int16_t* channel,
                          int64_t* timestamp, uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset, int32_t* n_samples,
                          int64_t* n_waves, int64_t* consumed_bytes);

/* Records stream: records and wave_pool from V1725 blocks, block by block (the streamed form of wfa_records_sort +
 * wfa_pool_gather over a run's files; reference: records_builder.py:797-830 `build_records_from_v1725_files`).  The device
 * keeps the waves a later block could still precede (the carry) and releases the others as RECORDS_DTYPE rows with their
 * samples, in the order of the static table: (timestamp, pid = 0, board, channel, seq).
 * A horizon H is an int64 (ps) such that every wave not yet pushed has timestamp >= H.
 * _begin(dt_ns): empty carry, next_record = next_sample = 0, horizon = the smallest int64.
 * _push takes a block's bytes (host memory; they go up through the pinned staging ring like wfa_upload_pool_u16) and the
 * n_waves new waves as columns: timestamp_ps i8 (ticks * dt_ns * 1000, formed by the caller), seq i8 (the caller's total
 * order of the waves: file index, then wave index in the file -- a sort key behind channel, since a carried wave of a later
 * file may tie with a pushed wave of an earlier one), payload_offset i8 (bytes into the block, a multiple of 4), n_samples
 * i4 (even, >= 0), board i2, channel i2, baseline u2, trunc u1.  n_waves = 0 (block may be NULL) is a pure flush.  Steps:
 * the new waves go behind the carried ones as 40-byte entries; the table is ordered by (timestamp, board, channel, seq)
 * with the radix sort of wfa_records_sort; the released waves are the prefix with timestamp < horizon_ps, strictly (a later
 * wave may tie at the horizon with a smaller board / channel), or the whole table when final != 0; the exclusive scan of
 * the lengths in that order gives wave_offset = next_sample + scan for the prefix and the offsets in the new sample carry
 * for the rest; ONE sample pass (k_rs_move) moves every wave's samples from where they are -- the old sample carry or the
 * block's bytes -- to where they go -- the output pool or the new sample carry; the released rows are written on the device
 * as packed 102-byte RECORDS_DTYPE rows: timestamp i8 @0, pid i4 @8 = 0, board i2 @12, channel i2 @14, baseline f8 @16 (the
 * header's uint16), baseline_upstream f8 @24 = NaN, polarity 8 x UCS-4 @32 = "unknown", record_id i8 @64 = next_record + k,
 * dt i4 @72, trigger_type i2 @76 = 0, flags u4 @78 = trunc, wave_offset i8 @82, event_length i4 @90, time i8 @94 =
 * floor(timestamp / 1000); the other entries are compacted into the other carry buffer.  Samples keep their int16 bit
 * patterns; a zero-sample wave moves nothing and still gets a row.
 * _push reports the records and samples released and those carried; _fill downloads the released rows and samples
 * (n_out_records x 102 bytes, n_out_samples x 2 bytes); the next push overwrites them.
 * Host waits of a push: one per key range of the sort, one for the counts, one when the push ends, and one more in a push
 * that has to grow a carry buffer; _fill waits for its copies.
 * Refused with WFA_E_INVALID, the stream left exactly as it was (every check is made on the host before anything is
 * uploaded): dt_ns <= 0 (_begin); a wave whose timestamp lies below the previous push's horizon; a horizon below the
 * previous one; a payload slice outside the block or not 4-byte aligned; a negative or odd n_samples; carry + pushed waves
 * >= 2^31.  _push without _begin, _fill before a push or after a refused one: WFA_E_STATE; _fill with other counts:
 * WFA_E_INVALID.  _begin on an open stream starts over.  A context may hold this stream open beside the event, merge,
 * merged-event and df_events streams.
 * State, not scratch: the entry carry (40 B per wave in each of two buffers), the sample carry (two buffers of the carried
 * samples), the rows and samples of the last push and the buffer of the last block: wfa_release_scratch keeps them,
 * wfa_scratch_bytes does not count them, _end frees them.  Scratch: the sort's keys and buffers, the scanned lengths. */
int wfa_records_stream_begin(wfa_ctx* ctx, int32_t dt_ns);
int wfa_records_stream_push(wfa_ctx* ctx, const uint8_t* block, int64_t n_bytes, int64_t n_waves, const int64_t* timestamp_ps,
                            const int64_t* seq, const int64_t* payload_offset, const int32_t* n_samples, const int16_t* board,
                            const int16_t* channel, const uint16_t* baseline, const uint8_t* trunc, int64_t horizon_ps,
                            int final, int64_t* n_out_records, int64_t* n_out_samples, int64_t* n_carry_records,
                            int64_t* n_carry_samples);
int wfa_records_stream_fill(wfa_ctx* ctx, void* out_rows, uint16_t* out_pool, int64_t n_out_records, int64_t n_out_samples);
int wfa_records_stream_end(wfa_ctx* ctx);

/* K6 integral-quantile width (reference: waveform_width_integral.py:166-227).
 * out: WAVEFORM_WIDTH_INTEGRAL_DTYPE rows (52 B). */
int wfa_width_integral(wfa_ctx* ctx, int source, double q_low, double q_high, double dt,
                       void* out_rows);

/* BasicFeaturesPlugin and WaveformWidthIntegralPlugin records branches (cpu/basic_features.py:108-195,
 * cpu/waveform_width_integral.py:83-231) on the raw wave_pool in ONE read of the pool: BASELINE config 3 asks for both
 * tables of the same records.  Uniform records, area range = whole record: one kernel stages every group of records once
 * and forms both rows (the same additions in the same order as the two separate kernels: identical bytes); any other
 * layout / range runs the two kernels one after the other.  out_basic (36-byte rows) / out_width (52-byte rows) may be NULL:
 * the tables then stay on the device only. */
int wfa_features_both(wfa_ctx* ctx, int64_t height_start, int64_t height_end, int height_has_end, int64_t area_start,
                      int64_t area_end, int area_has_end, double q_low, double q_high, double dt, void* out_basic,
                      void* out_width);

/* ---- measurement ------------------------------------------------------------------------ */

/* on = 1: every kernel launch is bracketed by HIP events on the ctx stream.  on = 2: only the streaming (mask) kernel
 * of the fused / SG-fused hit pass is -- the pair of events around each of its small follow-up kernels costs about as
 * much as the gap it measures.  on = 0: off. */
int wfa_profile_enable(wfa_ctx* ctx, int on);
int wfa_profile_reset(wfa_ctx* ctx);
/* idx-th profiled kernel: name (<= name_len), summed milliseconds, launches. Returns
 * WFA_E_INVALID past the end. */
int wfa_profile_get(wfa_ctx* ctx, int idx, char* name, size_t name_len, double* total_ms,
                    int64_t* launches);

/* ---- multi-GPU gather for event grouping (RCCL over xGMI) -------------------------------- */

/* 128-byte unique id created on rank 0 and broadcast by the launcher. */
int wfa_rccl_unique_id(void* id128);
int wfa_rccl_init(wfa_ctx* ctx, int rank, int n_ranks, const void* id128);
/* Step 1: every rank learns counts[n_ranks] (one int64 all-gather). */
int wfa_rccl_allgather_counts(wfa_ctx* ctx, int64_t n_rows, int64_t* counts);
/* Step 2: all ranks send n_rows rows of row_bytes each to `root` (grouped send/recv); the
 * root receives them concatenated in rank order into out (host buffer of sum(counts) rows,
 * ignored elsewhere).  rows == NULL sends the device-resident rows of the last hit pass
 * (row_bytes must be 60) without a host round trip.  counts = result of step 1. */
int wfa_rccl_gather_rows(wfa_ctx* ctx, const void* rows, int64_t n_rows, int32_t row_bytes,
                         int root, const int64_t* counts, void* out);
/* on != 0: the 60-byte rows of the following exchanges are appended on the root behind the rows already gathered (a rank
 * that works through several shards or time-range chunks sends one exchange per chunk; event grouping,
 * event_grouping.py:286-471, then reads one table: wfa_hit_rows_source(ctx, 2)).  `out` of such an exchange receives
 * only that exchange's rows.  on == 0: back to one table per exchange; the gathered table is dropped. */
int wfa_rccl_gather_append(wfa_ctx* ctx, int on);
int wfa_rccl_destroy(wfa_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* WFA_HIP_H */
