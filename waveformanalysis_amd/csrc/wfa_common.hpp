// Shared host-side definitions of libwfa_hip.so (context, error handling, buffer helpers).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wfa_hip.h"
#include "wfa_host.hpp"
#include "wfa_kernels.hpp"

namespace wfa {

extern thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...);

// host -> device on the context's stream: the pinned staging ring from 4 MiB on, a plain async copy below (wfa_capi.hip)
int h2d_copy(wfa_ctx* c, void* dst, const void* src, size_t bytes);
// device -> host through the same pinned ring: chunk k+1 is on the wire while the host copies chunk k out.  `queued`
// (may be null) runs once, right after the first chunk's copy is queued: work it enqueues overlaps the host's draining.
// Returns when every byte has reached dst (wfa_capi.hip)
int d2h_staged(wfa_ctx* c, void* dst, const void* src, size_t bytes, int (*queued)(void*), void* arg);

#define WFA_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return ::wfa::fail(WFA_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                               __FILE__, __LINE__);                                          \
    } while (0)

// Growable device buffer.
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    // a scratch buffer lists itself in its owner's `scratch` (wfa_ctx declares the list above its buffers, lives on the
    // heap and is never copied): what wfa_release_scratch gives back and wfa_scratch_bytes counts
    explicit DevBuf(std::vector<DevBuf*>& scratch) { scratch.push_back(this); }
    DevBuf(const DevBuf&) = delete;             // owns device memory
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }                    // (wfa_ctx_destroy: `delete c` frees every buffer of the context)
    int ensure(size_t bytes);  // keeps contents only if no growth is needed
    void release();
    template <typename T>
    T* as() const {
        return reinterpret_cast<T*>(ptr);
    }
};

// A stream's carry: a table of fixed-size rows in one of two buffers.  The first n rows of table() were left by the last
// accepted push; a push puts its rows behind them (reserve, upload), works on the whole table and compacts the rows that
// stay into the other buffer.  None of that touches cur or n: the caller commits once the whole push has succeeded, so a
// refused push leaves the carry as it was.  State, not scratch: wfa_release_scratch keeps the buffers (wfa_hits.hip)
struct Carry {
    DevBuf buf[2];
    int cur = 0;
    int64_t n = 0;   // rows carried
    const int row;   // bytes per row: 8, 40, 60 or 88
    explicit Carry(int row_bytes) : row(row_bytes) {}
    DevBuf& table() { return buf[cur]; }
    int reserve(wfa_ctx* c, int64_t n_new);                   // room for n + n_new rows, the carried ones kept
    int upload(wfa_ctx* c, const void* rows, int64_t n_new);  // host rows behind the carry (room reserved)
    // the flagged rows of the n_table rows of table(), n_keep of them (incl = the inclusive scan of flag), into the other
    // buffer in row order
    int compact(wfa_ctx* c, int64_t n_table, const int64_t* flag, const int64_t* incl, int64_t n_keep);
    void commit(int64_t n_keep, bool flip) { cur ^= flip ? 1 : 0; n = n_keep; }
    void clear() { cur = 0; n = 0; }  // an empty carry; the buffers are reused
    void release() { buf[0].release(); buf[1].release(); clear(); }
};

struct ProfEntry {
    std::string name;
    double total_ms = 0.0;
    int64_t launches = 0;
};

struct SgPlanDev {
    int W = 0, P = 0, H = 0;
    int n_tables = 0;
    int stride = 0;   // doubles per table
    int int_ok = 0;
    int32_t den = 1, den_edge = 1;
    int64_t guard = 0, guard_edge = 0;
    double rden = 1.0, rden_edge = 1.0;
    DevBuf tab;   // double
    DevBuf itab;  // int32
    DevBuf sym;   // uint8
    std::vector<uint8_t> sym_host;
};

// One fused hit pass (run_hits, wfa_capi.hip): what it reads besides the resident pool, the records' other columns and the
// route options of the context.  The single-pass entry points fill it from the context, the grouped pass once per group.
struct HitPass {
    int source = 0;
    const SgPlanDev* plan = nullptr;  // Savitzky-Golay plan (null: none)
    const double* thr = nullptr;      // device column the pass compares against, one threshold per record
    bool fused_bl = false;
    int32_t bl_start = 0, bl_end = 0, le = 0, re = 0, max_len = 0;
    int64_t hint = -1;                // rows of the previous pass like this one: sizes the speculative launch (-1: none)
    bool speculate = true;            // false: exact row launches (host round trip for the hit count)
    bool enqueue_only = false;        // queue the speculative launch and return without the count, where the pass can
    RunsCold* cold_pin = nullptr;     // pinned slot the streaming route's cold block is staged through
};

// What a pass did.  kNone: the streaming route declined (run_hits_runs32 alone).
struct HitOutcome {
    enum { kNone, kQueued, kCompleted } state = kNone;
    int64_t bound = 0;      // kQueued: rows the launches were sized for; the count is on its way to the pinned words
    bool runs32 = false;    // kQueued on the streaming route: the overflow flags come with the count
    int64_t n_hits = -1;    // kCompleted: rows in hit_out
    bool overflow = false;  // the streaming route found a span's events outgrowing their buffer
};

}  // namespace wfa

struct wfa_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<wfa::DevBuf*> scratch;  // the buffers declared `{scratch}` below, ht[] and dense_rows[]
    wfa_ctx() {
        for (wfa::DevBuf& b : ht) scratch.push_back(&b);
        for (wfa::DevBuf& b : dense_rows) scratch.push_back(&b);
    }

    // resident pool
    wfa::DevBuf pool_u16;
    wfa::DevBuf pool_f32;
    int64_t pool_n = 0;
    bool have_u16 = false, have_f32 = false;

    // records SoA
    int64_t R = 0;
    int32_t max_len = 0;
    bool have_records = false;
    wfa::DevBuf off, len, baseline, pol, thr, ts, dt, board, chan, rid, fixed_bl, bm_off;
    // host copy of `len`, fetched by the first wfa_view_gather after a records upload (it sizes and checks the rows
    // of a request before any launch)
    std::vector<int32_t> len_host;
    bool len_host_valid = false;
    int64_t bitmap_bytes = 0;  // mask bits of all records (k_sg_mask -> k_hit_runs)
    // what the records upload found about its layout (wfa_host.hpp), and whether the padded shadow of the u16 pool
    // (layout.pad: records at stride layout.S, with the matching offsets column) has been built for it: on the device, the
    // first time a pass needs it (layout_view, wfa_capi.hip)
    wfa::UniformLayout layout;
    bool shadow_valid = false;
    wfa::DevBuf shadow_pool{scratch}, shadow_off{scratch};
    bool bitmap_clean = false;  // padding bytes of the bitmap are zero

    wfa::SgPlanDev sg;
    bool have_sg = false;
    bool filter_keep = false;  // wfa_filter_keep_output

    // hit scratch
    wfa::DevBuf hit_tmp{scratch};  // 60 B rows in chunk order
    int64_t hit_tmp_rows = 0;
    wfa::DevBuf cursor;         // unsigned long long
    wfa::DevBuf rec_tmp_start;  // int64 per record
    wfa::DevBuf rec_nhits;      // int32 per record
    wfa::DevBuf rec_out_start;  // int64 per record
    wfa::DevBuf scan_blocks;    // int64 per scan block
    wfa::DevBuf hit_out;        // final rows
    wfa::DevBuf bitmap{scratch};  // 1 bit per sample, per-record regions (bm_off)
    wfa::DevBuf hit_desc;       // int4 (record, start, end, k) per hit
    // streaming pass on uniform records (k_sg_runs32): event buffer, per-span tables, control words
    wfa::DevBuf run_ev{scratch}, run_span_off, run_span_cnt, run_span_row0, run_scan_blocks, run_ctrl, run_groups, run_lit;
    // host -> device staging: two pinned buffers; a chunk is copied in (a few host threads) while the previous one is on
    // the wire.  Pageable hipMemcpyAsync of a whole pool depends on the driver's own staging (5 GB/s on one box, 0.03
    // GB/s on another)
    void* stage[2] = {nullptr, nullptr};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    size_t stage_bytes = 0;
    double last_h2d_GBps = 0.0;  // rate of the last staged upload (wfa_last_h2d_rate)
    // wfa_upload_dense_rows: two buffers of packed rows, the second stream k_dense_unpack runs on while the next batch
    // is copied on `stream`, one event per buffer (its unpack has finished) and one for "the copy has landed"; the
    // stream and the events are created by the first dense upload
    wfa::DevBuf dense_rows[2];
    wfa::DevBuf dense_neg;  // int64: first row with a negative sample
    hipStream_t dense_stream = nullptr;
    hipEvent_t dense_ev[3] = {nullptr, nullptr, nullptr};

    // wfa_set_option: choice between code paths that give identical results (tests compare them; a caller never needs to)
    struct {
        bool no_fast = false;      // literal float64 k_hits instead of the integer kernels
        bool no_span = false;      // per-record mask kernel instead of the uniform-record kernels
        bool no_pad = false;       // no padded shadow layout
        bool no_runs32 = false;    // bitmap route (k_sg_mask_span16 + scan + k_hit_runs) instead of k_sg_runs32
        bool no_speculate = false; // exact row launches (host round trip for the hit count)
        bool no_deposit = false;    // streaming kernel: the flush reads the records' last samples from memory again (no LDS deposit)
        int span_records = 0;       // streaming kernel: records per span (measurement; 0 = library's choice)
        bool no_peak_hot = false;   // find_peaks: the plateau machine over every sample (k_find_peaks_staged), no height prefilter
        bool no_peak_slots = false; // find_peaks: count + fill walks instead of one walk into per-record slots
    } opt;
    wfa::RunsCold* h_cold = nullptr;   // pinned staging (lives behind h_total)
    wfa::RunsCold run_cold_host{};     // what the device copy holds
    bool run_cold_valid = false;
    bool no_runs32 = false;   // a span outgrew the event buffer of its wave: this records upload takes the general route
    int64_t n_hits = -1;
    // rows of the last single pass with a row stage, or the merged total of the last grouped call: the hint of the next
    // single pass (HitPass::hint).  Written by the entry points and by the settle step of wfa_hits_wait, never by a pass
    int64_t last_hits = -1;
    // where the record index of every row of the last hit pass stands: 0 nowhere (no pass yet, a merged table, or the
    // per-record buffers taken by another stage), 1 hit_desc[i].x (streaming and bitmap routes), 2 rec_nhits /
    // rec_out_start (general route: per-record counts and their exclusive scan)
    int rows_index = 0;
    // stash of a grouped pass (wfa_hits_enqueue_groups): the rows of the groups' passes back to back, the record index of
    // every row, and the final place of every row in the merged table
    wfa::DevBuf merge_rows{scratch}, merge_rec{scratch}, merge_dest{scratch};
    // resident plan slots (wfa_sg_plan_store): one Savitzky-Golay plan per filter group of a grouped pass, kept across
    // pool and records uploads like `sg`
    wfa::SgPlanDev sg_slot[WFA_MAX_HIT_GROUPS];
    bool have_slot[WFA_MAX_HIT_GROUPS] = {};
    // the last grouped pass (wfa_hits_enqueue_groups): its arguments, all a queued one (pending == kPendGroups) keeps for
    // wfa_hits_wait and its exact redo; per group the outcome of its pass -- the row bound its launches were sized for
    // (queued) or the row count the host already read (n_host >= 0) -- and `last`, the row count of the group's previous
    // pass on this context (the hint of its next one; -1: none yet)
    struct GroupsPass {
        bool single = false;   // one group, no unowned record: the plain pass with the slot's plan
        int n_groups = 0;
        int64_t R = -1;        // records the pass was queued over (the redo needs the same table)
        wfa_hit_group groups[WFA_MAX_HIT_GROUPS] = {};
        int32_t bl_start = 0, bl_end = 0;  // baseline window of the WFA_SRC_SG_FUSED groups (bl_end <= bl_start: none)
        int32_t le = 0, re = 0, max_len = 0;
        int64_t bound[WFA_MAX_HIT_GROUPS] = {};
        int64_t n_host[WFA_MAX_HIT_GROUPS] = {};
        bool runs32[WFA_MAX_HIT_GROUPS] = {};
        int64_t last[WFA_MAX_HIT_GROUPS] = {-1, -1, -1, -1, -1, -1, -1, -1};
    } grp;
    wfa::DevBuf grp_gor;   // int32 per record: group_of_record of the last grouped pass
    wfa::DevBuf grp_thr;   // double per record: own-or-+inf copy of the threshold column, what the current group's pass compares against
    wfa::DevBuf grp_sets;  // int64 [WFA_MAX_HIT_GROUPS + 1] stash offsets written on the device, then [fail flag]
    // pinned: per group (row count, overflow flags), the stash offsets as the device wrote them, the merged count and
    // the fail flag; behind them one RunsCold per group (what k_sg_runs32's float64 paths read under that group's plan)
    int64_t* h_grp = nullptr;
    wfa::RunsCold* h_grp_cold = nullptr;

    wfa::DevBuf out_rows;  // per-record feature rows
    wfa::DevBuf out_rows2; // the second table of wfa_features_both (width rows)
    wfa::DevBuf pw_plan;   // numpy pairwise-sum plan of the wave-per-record feature kernels (wfa_features.hip)
    int pw_plan_n = -1;    // reduction length the device copy was built for
    wfa::DevBuf fw_ties{scratch};  // width-integral records whose quantile positions are re-walked in numpy's order
    wfa::DevBuf peak_out;  // HIT_DTYPE rows of the last find_peaks pass
    int64_t n_peaks = -1;
    int peak_mode = 0;      // WFA_PEAK_SIGNAL_* of the pass that wrote peak_out
    // records_gen counts the records tables this context has held (every upload and every drop); peak_gen is its value
    // when peak_out was written: the peak chain evaluates the rows only on the table they were found on
    int64_t records_gen = 0, peak_gen = -1;
    // peak chain (wfa_peak_chain_count): feature rows of the records, one row slot per peak, the kept rows
    wfa::DevBuf pc_feat{scratch}, pc_rows{scratch}, pc_out{scratch};
    int64_t n_chain = -1;   // kept rows of the last peak chain pass; -1: none, or its scratch was released
    int64_t n_legacy = -1;  // hits of the last wfa_find_hits_count pass
    wfa::DevBuf peak_cand_n{scratch}, peak_cand_pos{scratch}, peak_cand_val{scratch}, peak_cand_state{scratch};  // candidate lists of find_peaks
    wfa::DevBuf peak_slot_pos{scratch}, peak_slot_val{scratch};  // kPeakSlots candidates per record, written by the single walk
    wfa::DevBuf peak_cand_rec{scratch}, peak_accept{scratch}, peak_ips{scratch}, peak_row_start{scratch};
    wfa::DevBuf wh_pos{scratch}, wh_row{scratch}, wh_valid{scratch};  // per-hit inputs of k_waveform_width
    // hit-table stages (wfa_hits.hip): scratch slots and the state of the last count pass
    wfa::DevBuf ht[48];
    int ht_src = 1;            // wfa_hit_rows_source: 1 = rows of the last hit pass, 2 = rows of the last gather
    wfa::DevBuf gathered;      // rows the last wfa_rccl_gather_rows left on the root
    int64_t gathered_n = -1;
    bool gather_append = false;  // wfa_rccl_gather_append: exchanges add to the gathered table instead of replacing it
    int64_t ht_n = -1, ht_groups = 0;
    int ht_kind = 0;  // 1 = event grouping, 2 = hit merge, 3 = legacy multi-channel grouping
    int64_t* ht_perm = nullptr;
    // CSV decode (wfa_hits.hip): rows / samples of the last wfa_csv_decode_count pass; the samples stay resident
    int64_t csv_rows = -1, csv_samples = -1, csv_bytes = 0;
    int32_t csv_samples_start = 0;
    int csv_delim = ';';
    bool csv_filled = false;
    // sample arena of a run decoded in several parts (wfa_csv_arena_*): part k's samples land at [base_k, base_k + n_k);
    // [0, arena_filled) has been written.  Not scratch: wfa_release_scratch keeps it, wfa_ctx_destroy frees it
    wfa::DevBuf csv_arena;
    int64_t arena_filled = 0;
    // The carry streams (wfa_*_stream_*, wfa_hits.hip).  Each is a run's settings and counters (a `Run`, which _begin starts
    // over), the rows still open after the last accepted push in a wfa::Carry, and what that push closed in an output
    // buffer until _fill takes it.  out_* < 0: nothing to fill (no push yet, or the last one was refused).  A context may
    // hold all four open side by side.  State, not scratch: wfa_release_scratch keeps the buffers, _end releases them.
    template <typename Run>
    struct GroupStream : Run {  // one carry, one output table: the event stream and the df_events stream
        wfa::Carry carry;
        wfa::DevBuf out;
        explicit GroupStream(int entry_bytes) : carry(entry_bytes) {}
        void restart() { Run::operator=(Run{}); carry.clear(); }  // (the buffers are reused)
        void release() { restart(); carry.release(); out.release(); }
    };
    // event stream: the hits of the open events as 60-byte rows; a push closes 84-byte rows
    struct EventRun {
        bool open = false;
        double window_ns = 0.0;
        double horizon = 0.0;     // horizon of the last accepted push (-inf before the first)
        int64_t next_event = 0;   // events emitted so far = id of the next one
        int64_t out_rows = -1;    // rows of the last push waiting in `out`
    };
    using EventStream = GroupStream<EventRun>;
    EventStream es{60};
    // merge stream: the hits of the open clusters as 60-byte rows, each row's index in the sequence of all pushed rows
    // beside it in a second carry compacted under the same flag; a push closes 72-byte merged rows and their members' indices
    struct MergeRun {
        bool open = false;
        double gap_ns = 0.0, width_ns = 0.0;
        double horizon = 0.0;       // horizon of the last accepted push (-inf before the first)
        int64_t next_hit = 0;       // rows pushed so far = index of the next pushed row
        int64_t next_component = 0; // component rows emitted so far = component_offset of the next cluster
        int64_t out_merged = -1, out_components = 0;  // of the last push, waiting in out / out_index
    };
    struct MergeStream : MergeRun {
        wfa::Carry carry{60}, index{8};
        wfa::DevBuf out, out_index;
        void restart() { MergeRun::operator=(MergeRun{}); carry.clear(); index.clear(); }
        void release() { restart(); carry.release(); index.release(); out.release(); out_index.release(); }
    } ms;
    // merged-event stream: a merge step and a group step per push, each on the state of the stream it is the body of.  The
    // merged rows go straight behind the event carry (m.out stays empty), whose entries are 88 bytes: a 72-byte merged row,
    // then its abs_start_fix / abs_end_fix.  A push closes 96-byte rows (e.out) and member indices (m.out_index), both
    // waiting while e.out_rows >= 0.  e.horizon is the grouping horizon G of the last push
    struct MergedEventStream {
        bool open = false;
        double margin_ps = 0.0;   // the run's horizon margin (2 ulp of its magnitude; 0 below 2^53 ps)
        MergeStream m;
        EventStream e{88};
        void restart() { open = false; margin_ps = 0.0; m.restart(); e.restart(); }
        void release() { restart(); m.release(); e.release(); }
    } mes;
    // df_events stream: the fixed-window grouping chunk by chunk.  The rows of the open events as 40-byte DF_ROW_DTYPE
    // rows; a push closes 64-byte rows
    struct DfEventRun {
        bool open = false;
        double window_ps = 0.0;
        int64_t horizon = INT64_MIN;  // horizon of the last accepted push (the smallest int64 before the first)
        int64_t next_event = 0;       // events emitted so far = id of the next one
        int64_t out_rows = -1;        // rows of the last push waiting in `out`
    };
    using DfEventStream = GroupStream<DfEventRun>;
    DfEventStream ds{40};
    // records stream (wfa_records_stream_*): the head of the chain.  The waves a later block could still precede: a fixed
    // 40-byte entry each in `carry` (timestamp, seq, offset of its samples in the sample carry, n_samples | board | channel,
    // baseline | trunc) and their samples back to back in samples[cur_s] -- a second pair of ping-pong buffers, flipped with
    // the carry once a whole push has succeeded.  A push releases RECORDS_DTYPE rows (out_rows) and their samples (out_pool)
    struct RecordsRun {
        bool open = false;
        int32_t dt_ns = 0;
        int64_t horizon = INT64_MIN;   // horizon of the last accepted push (the smallest int64 before the first)
        int64_t next_record = 0;       // records released so far = record_id of the next one
        int64_t next_sample = 0;       // samples released so far = wave_offset of the next record
        int64_t out_records = -1;      // of the last push, waiting in out_rows / out_pool
        int64_t out_samples = 0;
    };
    struct RecordsStream : RecordsRun {
        wfa::Carry carry{40};
        wfa::DevBuf samples[2];
        int cur_s = 0;
        int64_t n_samples = 0;         // samples carried
        wfa::DevBuf out_rows, out_pool;
        wfa::DevBuf block;             // the bytes of the block being pushed (dead once the push returns)
        std::vector<int64_t> pack;     // host: the pushed waves as carry entries, until their upload has been queued
        void restart() { RecordsRun::operator=(RecordsRun{}); carry.clear(); cur_s = 0; n_samples = 0; }
        void release() {
            restart(); carry.release(); samples[0].release(); samples[1].release(); out_rows.release(); out_pool.release();
            block.release(); pack = {};
        }
    } rs;
    wfa::DevBuf bw_scratch{scratch};  // float64 forward pass of sosfiltfilt, [sample][record-in-batch]

    // profiling: HIP events around every launch on the context's stream.  The pairs are only recorded while the
    // work runs and resolved (hipEventElapsedTime) when the report is read, so timing adds no host round trip
    // between the kernels of a pass.
    bool prof_on = false;
    int prof_level = 0;  // 0 off, 1 every launch, 2 dominant kernels only
    std::vector<wfa::ProfEntry> prof;
    struct PendingEvent {
        hipEvent_t e0, e1;
        std::string name;
    };
    std::vector<PendingEvent> prof_pending;
    std::vector<hipEvent_t> prof_free;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // enqueue-only hit passes (wfa_hits_enqueue / wfa_hits_wait): the row count of the last enqueued pass lands in a
    // pinned host word
    int64_t* h_total = nullptr;
    // streaming route: the group sums [0, run_dirty_groups) of run_groups, and with any of them the two control words of
    // run_ctrl, may be non-zero.  Raised before k_sg_runs32, lowered only once a clear of the whole extent is enqueued.
    int64_t run_dirty_groups = 0;
    // what wfa_hits_wait has to settle: nothing, a single pass (`pend`) or a grouped one (`grp`)
    enum Pending { kPendNone = 0, kPendPass, kPendGroups } pending = kPendNone;
    // queued single pass: its description, kept for the exact redo, and what it reported (bound, runs32)
    struct PendingPass { wfa::HitPass pass; wfa::HitOutcome out; } pend{};

    // rccl (opaque, owned by wfa_rccl.hip)
    void* comm = nullptr;
    int rank = 0, n_ranks = 1;
};

namespace wfa {

// ---- what an upload voids: every entry point that replaces the pool or the records says so here, and only here ----
// what a pass builds in scratch for the resident records and keeps for the next one: gone with the records or the scratch
inline void pass_caches_dropped(wfa_ctx* c) { c->shadow_valid = c->bitmap_clean = false; }

// No records: the passes refuse until the next records upload, and what the old ones gave rise to goes with them.
inline void records_dropped(wfa_ctx* c) {
    c->have_records = false;
    c->records_gen += 1;
    c->layout = {};
    pass_caches_dropped(c);
}

// A records upload has landed: nothing cached for the previous table survives.
inline void records_replaced(wfa_ctx* c, int64_t R, int32_t max_len, int64_t bitmap_bytes, const UniformLayout& layout) {
    c->R = R; c->max_len = max_len; c->bitmap_bytes = bitmap_bytes; c->layout = layout;
    c->have_records = true;
    c->records_gen += 1;
    pass_caches_dropped(c);
    c->len_host_valid = c->no_runs32 = false;
    c->n_hits = c->pw_plan_n = -1;
}

// A pool of n samples has landed.  A wave_pool (u16) starts a new run: the filtered pool and the records belonged to the
// previous one.  A float32 pool beside a wave_pool (of equal size: the caller has dropped any other) is its filtered
// twin and the records stay; alone it is the run.
inline void pool_replaced(wfa_ctx* c, int64_t n, bool u16) {
    if (u16) {
        c->have_u16 = true;
        c->have_f32 = c->filter_keep = false;
    } else {
        c->have_f32 = true;
        if (c->have_u16) return;
    }
    c->pool_n = n;
    records_dropped(c);
}

// Launch timer: constructed before the launch(es), end(name) after them.
struct LaunchTimer {
    wfa_ctx* c;
    hipEvent_t e0 = nullptr;
    static hipEvent_t take(wfa_ctx* c) {
        if (!c->prof_free.empty()) {
            hipEvent_t e = c->prof_free.back();
            c->prof_free.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    // dominant: the kernel the roofline figure is about -- the only one timed at profile level 2, where the event
    // pairs around the small kernels of a pass would cost as much as the gaps they measure
    explicit LaunchTimer(wfa_ctx* ctx, bool dominant = false) : c(ctx) {
        if (!c->prof_on || (c->prof_level == 2 && !dominant)) return;
        e0 = take(c);
        if (e0) (void)hipEventRecord(e0, c->stream);
    }
    int end(const char* name) {
        if (!c->prof_on || !e0) return WFA_OK;
        hipEvent_t e1 = take(c);
        if (!e1) { c->prof_free.push_back(e0); e0 = nullptr; return WFA_OK; }
        WFA_HIP_CHECK(hipEventRecord(e1, c->stream));
        c->prof_pending.push_back({e0, e1, name});
        e0 = nullptr;
        return WFA_OK;
    }
};

// resolve the recorded pairs into the per-name totals (blocks until the last recorded event has completed)
inline int profile_flush(wfa_ctx* c) {
    for (auto& p : c->prof_pending) {
        float ms = 0.f;
        hipError_t err = hipEventSynchronize(p.e1);
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, p.e0, p.e1);
        c->prof_free.push_back(p.e0);
        c->prof_free.push_back(p.e1);
        if (err != hipSuccess) continue;
        bool found = false;
        for (auto& e : c->prof)
            if (e.name == p.name) { e.total_ms += ms; e.launches += 1; found = true; break; }
        if (!found) c->prof.push_back({p.name, (double)ms, 1});
    }
    c->prof_pending.clear();
    return WFA_OK;
}

}  // namespace wfa
