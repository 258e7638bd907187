// Hit-table stages on the device: hit merging (cpu/hit_merge.py) and event grouping
// (processing/event_grouping.py:286-471).  These are the reduce steps after the sample kernels: tables of
// 10^5..10^7 hit rows, sorted with rocPRIM's stable radix sort (through hipCUB) and reduced with scans and
// small per-group / per-cluster kernels.  Multi-key orders are built the way np.lexsort defines them:
// stable sorts from the least significant key to the most significant one.
#include <cstring>

#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/functional.hpp>

#include "wfa_common.hpp"
#include "wfa_host.hpp"
#include "wfa_numpy.hpp"

namespace wfa {
namespace {

constexpr int kTB = 256;

__device__ __forceinline__ uint64_t ord_f64(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t ord_i64(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + kTB - 1) / kTB); }

// ---- scratch slots of wfa_ctx::ht ------------------------------------------------------------------------
enum Slot {
    S_TS, S_POS, S_START, S_END, S_DT, S_BOARD, S_CHAN, S_RID, S_HEIGHT, S_INTEGRAL,
    S_ABS0, S_ABS1, S_K0, S_K1, S_K2, S_K3, S_K4, S_KTMP0, S_KTMP1, S_PERM0, S_PERM1, S_CUB,
    S_F0, S_F1, S_FLAG, S_ID, S_OUT0, S_OUT1, S_OUT2, S_OUT3, S_OUT4, S_OUT5, S_OUT6, S_OUT7, S_CNT, S_CNT2, S_SG, S_CSV, S_ES, S_EVHI,
    S_MS0, S_MS1, S_MS2, S_MS3, S_MS4, S_MS5, S_MS6, S_N
};
static_assert(S_N <= 48, "wfa_ctx::ht is too small");

template <typename T>
int slot(wfa_ctx* c, int s, int64_t n, T** out) {
    int rc = c->ht[s].ensure((size_t)(n > 0 ? n : 1) * sizeof(T));
    if (rc) return rc;
    *out = c->ht[s].as<T>();
    return WFA_OK;
}

template <typename T>
int upload(wfa_ctx* c, int s, const T* host, int64_t n, T** dev) {
    int rc = slot<T>(c, s, n, dev);
    if (rc) return rc;
    if (n > 0) WFA_HIP_CHECK(hipMemcpyAsync(*dev, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return WFA_OK;
}

__global__ void k_iota(int64_t n, int64_t* p) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) p[i] = i;
}
__global__ void k_gather_u64(int64_t n, const uint64_t* __restrict__ src, const int64_t* __restrict__ perm,
                             uint64_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// min / max of up to 8 key columns in one pass (block reduce, then 64-bit atomics): mm[2k] = min, mm[2k + 1] = max
constexpr int kMaxSortKeys = 8;
struct KeyCols {
    const uint64_t* k[kMaxSortKeys];
    int n;
};
__global__ __launch_bounds__(kTB) void k_key_ranges(int64_t n, KeyCols kc, unsigned long long* __restrict__ mm) {
    __shared__ unsigned long long s_min[kTB / 64], s_max[kTB / 64];
    for (int q = 0; q < kc.n; ++q) {
        unsigned long long lo = ~0ull, hi = 0ull;
        for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
            const unsigned long long v = kc.k[q][i];
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        for (int d = 32; d > 0; d >>= 1) {
            const unsigned long long ol = __shfl_xor(lo, d), oh = __shfl_xor(hi, d);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if ((threadIdx.x & 63) == 0) { s_min[threadIdx.x >> 6] = lo; s_max[threadIdx.x >> 6] = hi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kTB / 64; ++w) { lo = s_min[w] < lo ? s_min[w] : lo; hi = s_max[w] > hi ? s_max[w] : hi; }
            atomicMin(&mm[2 * q], lo);
            atomicMax(&mm[2 * q + 1], hi);
        }
        __syncthreads();
    }
}
__global__ void k_gather_rebased(int64_t n, const uint64_t* __restrict__ src, const int64_t* __restrict__ perm,
                                 uint64_t base, uint64_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]] - base;
}

// perm <- the stable lexicographic order of keys[0] (primary), keys[1], ... ; returns the buffer holding it.
// Every key is sorted on (key - min) over the bits its range needs: a radix pass costs the same whatever the values
// are, and most keys are narrow (dt, board / channel, pid: a few bits or constant; timestamps in ps: ~45 bits).  A
// constant key is skipped.  One extra pass over the keys and one host round trip buy back a third to two thirds of
// the radix passes.
// init_perm (one of this function's own result buffers, or null = the identity): the order the stable passes start from --
// sorting an earlier result by a few more significant keys costs only those keys' passes.
int lexsort(wfa_ctx* c, int64_t n, const uint64_t* const* keys, int n_keys, int64_t** perm_out,
            const int64_t* init_perm = nullptr) {
    int rc;
    int64_t *p0, *p1;
    uint64_t *k0, *k1;
    if (n_keys > kMaxSortKeys) return fail(WFA_E_INVALID, "too many sort keys");
    if ((rc = slot<int64_t>(c, S_PERM0, n, &p0)) || (rc = slot<int64_t>(c, S_PERM1, n, &p1))) return rc;
    if ((rc = slot<uint64_t>(c, S_KTMP0, n, &k0)) || (rc = slot<uint64_t>(c, S_KTMP1, n, &k1))) return rc;
    if (n > 0x7fffffff) return fail(WFA_E_LIMIT, "hit table has %lld rows; the device sort handles < 2^31", (long long)n);
    unsigned long long* d_mm;
    if ((rc = slot<unsigned long long>(c, S_CNT, 2 * kMaxSortKeys, &d_mm))) return rc;
    unsigned long long mm[2 * kMaxSortKeys];
    for (int k = 0; k < kMaxSortKeys; ++k) { mm[2 * k] = ~0ull; mm[2 * k + 1] = 0ull; }
    WFA_HIP_CHECK(hipMemcpyAsync(d_mm, mm, sizeof(mm), hipMemcpyHostToDevice, c->stream));
    KeyCols kc{};
    kc.n = n_keys;
    for (int k = 0; k < n_keys; ++k) kc.k[k] = keys[k];
    const unsigned rb = blocks_for(n) < 1024u ? blocks_for(n) : 1024u;
    hipLaunchKernelGGL(k_key_ranges, dim3(rb), dim3(kTB), 0, c->stream, n, kc, d_mm);
    if (init_perm == p1) { int64_t* t = p0; p0 = p1; p1 = t; }  // the starting order already sits in a result buffer
    else if (init_perm && init_perm != p0) return fail(WFA_E_INVALID, "lexsort: init_perm must be an earlier result");
    if (!init_perm) hipLaunchKernelGGL(k_iota, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, p0);
    WFA_HIP_CHECK(hipMemcpyAsync(mm, d_mm, sizeof(mm), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    rocprim::double_buffer<uint64_t> kb(k0, k1);
    rocprim::double_buffer<int64_t> pb(p0, p1);
    size_t tmp_bytes = 0;
    WFA_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, pb, (size_t)n, 0u, 64u, c->stream));
    if ((rc = c->ht[S_CUB].ensure(tmp_bytes))) return rc;
    for (int k = n_keys - 1; k >= 0; --k) {
        const unsigned long long span = mm[2 * k + 1] - mm[2 * k];
        if (span == 0) continue;  // constant key: the order does not change
        const int bits = 64 - __builtin_clzll(span);
        hipLaunchKernelGGL(k_gather_rebased, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, keys[k], pb.current(),
                           (uint64_t)mm[2 * k], kb.current());
        size_t tb = c->ht[S_CUB].cap;
        WFA_HIP_CHECK(rocprim::radix_sort_pairs(c->ht[S_CUB].ptr, tb, kb, pb, (size_t)n, 0u, (unsigned)bits, c->stream));
    }
    WFA_HIP_CHECK(hipGetLastError());
    *perm_out = pb.current();
    return WFA_OK;
}

struct MaxF64 {
    __device__ double operator()(double a, double b) const { return b > a ? b : a; }
};

// ---- shared prep: absolute windows and sort keys ------------------------------------------------------------
struct HitCols {
    const int64_t* ts;
    const int64_t* pos;
    const int32_t* s;
    const int32_t* e;
    const int32_t* dt;
    const int16_t* board;
    const int16_t* chan;
    const int64_t* rid;
};

// abs = float(timestamp) + (float(edge) - float(position)) * (float(dt) * 1e3)
// (hit_merge.py:75-82, event_grouping.py:365-367; no contraction: the build uses -ffp-contract=off)
// Sort keys.  The window starts are float64 in the reference, but they are integers (picoseconds) whenever timestamps and
// dt are: then the key is that integer -- lexsort sorts (key - min) over the bits the range needs, 44 bits for 12 s of data
// where the float64 bit pattern needs 56 -- and the timestamp key, which only ever breaks ties between EQUAL starts, is
// (timestamp - start): a few thousand samples of range instead of the run's.  A start that is not an integer of magnitude
// below 4.0e18 raises *inexact: the caller rewrites the two keys in their float64 / plain forms (k_float_keys).
__global__ void k_hit_prep(int64_t n, HitCols h, const double* __restrict__ fix0, const double* __restrict__ fix1,
                           double* __restrict__ abs0, double* __restrict__ abs1,
                           uint64_t* __restrict__ k_abs0, uint64_t* __restrict__ k_dt, uint64_t* __restrict__ k_ts,
                           uint64_t* __restrict__ k_rid, uint64_t* __restrict__ k_chan, int* __restrict__ inexact) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const double t = (double)h.ts[i], p = (double)h.pos[i], dps = (double)h.dt[i] * 1e3;
    double a0 = t + ((double)h.s[i] - p) * dps, a1 = t + ((double)h.e[i] - p) * dps;
    if (fix0 && fix0[i] == fix0[i]) a0 = fix0[i];
    if (fix1 && fix1[i] == fix1[i]) a1 = fix1[i];
    abs0[i] = a0;
    abs1[i] = a1;
    const bool small = fabs(a0) < 4.0e18;
    const int64_t ai = small ? (int64_t)a0 : 0;
    if (!small || (double)ai != a0) atomicOr(inexact, 1);
    k_abs0[i] = ord_i64(ai);
    if (k_dt) k_dt[i] = (uint64_t)(uint32_t)h.dt[i];
    if (k_ts) k_ts[i] = ord_i64(h.ts[i] - ai);
    if (k_rid) k_rid[i] = ord_i64(h.rid[i]);
    // (board, channel[, dt]) ascending as signed integers
    const uint64_t bc = ((uint64_t)(uint16_t)(h.board[i] ^ (int16_t)0x8000) << 48) |
                        ((uint64_t)(uint16_t)(h.chan[i] ^ (int16_t)0x8000) << 32);
    k_chan[i] = k_dt ? (bc | (uint64_t)(uint32_t)h.dt[i]) : bc;
}

__global__ void k_float_keys(int64_t n, const double* __restrict__ abs0, const int64_t* __restrict__ ts,
                             uint64_t* __restrict__ k_abs0, uint64_t* __restrict__ k_ts) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    // np.lexsort compares float64 values: -0.0 == +0.0 is a tie the later keys decide, while the bit patterns differ
    // (a start of -0.0 can only come in through abs_start_fix).  The key is canonical; abs0 itself stays as given.
    const double v = abs0[i];
    k_abs0[i] = ord_f64(v == 0.0 ? 0.0 : v);
    if (k_ts) k_ts[i] = ord_i64(ts[i]);
}

// k_hit_prep + the check of its integer keys (one small device -> host copy)
int hit_prep(wfa_ctx* c, int64_t n, const HitCols& h, const double* fix0, const double* fix1, double* abs0, double* abs1,
             uint64_t* k_abs, uint64_t* k_dt, uint64_t* k_ts, uint64_t* k_rid, uint64_t* k_chan) {
    int rc;
    int* d_flag;
    if ((rc = slot<int>(c, S_CNT2, 4, &d_flag))) return rc;
    WFA_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_hit_prep, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, h, fix0, fix1, abs0, abs1, k_abs, k_dt, k_ts,
                       k_rid, k_chan, d_flag);
    int inexact = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&inexact, d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (inexact) hipLaunchKernelGGL(k_float_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, abs0, h.ts, k_abs, k_ts);
    return WFA_OK;
}

int upload_cols(wfa_ctx* c, int64_t n, const int64_t* ts, const int64_t* pos, const int32_t* s, const int32_t* e,
                const int32_t* dt, const int16_t* board, const int16_t* chan, const int64_t* rid, HitCols* h) {
    int rc;
    int64_t *d_ts, *d_pos, *d_rid;
    int32_t *d_s, *d_e, *d_dt;
    int16_t *d_b, *d_c;
    if ((rc = upload(c, S_TS, ts, n, &d_ts)) || (rc = upload(c, S_POS, pos, n, &d_pos)) ||
        (rc = upload(c, S_START, s, n, &d_s)) || (rc = upload(c, S_END, e, n, &d_e)) ||
        (rc = upload(c, S_DT, dt, n, &d_dt)) || (rc = upload(c, S_BOARD, board, n, &d_b)) ||
        (rc = upload(c, S_CHAN, chan, n, &d_c)) || (rc = upload(c, S_RID, rid, n, &d_rid)))
        return rc;
    *h = HitCols{d_ts, d_pos, d_s, d_e, d_dt, d_b, d_c, d_rid};
    return WFA_OK;
}

// Columns out of device-resident THRESHOLD_HIT_DTYPE rows (60 B packed: position i8 @0, edge_start i4 @16, edge_end i4
// @20, dt i4 @28, timestamp i8 @40, board i2 @48, channel i2 @50, record_id i8 @52; cpu/hit_finder.py:33-49): the rows
// of the last hit pass or of the last RCCL gather feed the hit-table stages without a host round trip.  `stride` = bytes
// from row to row (a multiple of 4): 60 for packed hit rows; the first 60 bytes of a HIT_MERGED_DTYPE row have the same
// layout (sample_start / sample_end where the edges stand), so the merged-event stream reads its 88-byte carry entries here.
__global__ void k_unpack_hit_rows(int64_t n, const uint8_t* __restrict__ rows, int64_t stride, int64_t* __restrict__ ts,
                                  int64_t* __restrict__ pos, int32_t* __restrict__ s, int32_t* __restrict__ e,
                                  int32_t* __restrict__ dt, int16_t* __restrict__ board, int16_t* __restrict__ chan,
                                  int64_t* __restrict__ rid) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const uint32_t* w = reinterpret_cast<const uint32_t*>(rows + i * stride);
    pos[i] = (int64_t)(((uint64_t)w[1] << 32) | w[0]);
    s[i] = (int32_t)w[4];
    e[i] = (int32_t)w[5];
    dt[i] = (int32_t)w[7];
    ts[i] = (int64_t)(((uint64_t)w[11] << 32) | w[10]);
    board[i] = (int16_t)(w[12] & 0xffffu);
    chan[i] = (int16_t)(w[12] >> 16);
    rid[i] = (int64_t)(((uint64_t)w[14] << 32) | w[13]);
}

// resident rows selected by wfa_hit_rows_source: 1 = rows of the last hit pass, 2 = rows of the last RCCL gather
int resident_cols(wfa_ctx* c, int64_t n, HitCols* h) {
    const uint8_t* rows = nullptr;
    int64_t have = -1;
    if (c->ht_src == 2) { rows = c->gathered.as<uint8_t>(); have = c->gathered_n; }
    else { rows = c->hit_out.as<uint8_t>(); have = c->pending ? -1 : c->n_hits; }
    if (have < 0) return fail(WFA_E_STATE, "no device-resident hit rows (run a hit pass / a gather first)");
    if (n != have) return fail(WFA_E_INVALID, "the resident hit table has %lld rows, the caller expects %lld", (long long)have, (long long)n);
    int rc;
    int64_t *d_ts, *d_pos, *d_rid;
    int32_t *d_s, *d_e, *d_dt;
    int16_t *d_b, *d_c;
    if ((rc = slot(c, S_TS, n, &d_ts)) || (rc = slot(c, S_POS, n, &d_pos)) || (rc = slot(c, S_START, n, &d_s)) ||
        (rc = slot(c, S_END, n, &d_e)) || (rc = slot(c, S_DT, n, &d_dt)) || (rc = slot(c, S_BOARD, n, &d_b)) ||
        (rc = slot(c, S_CHAN, n, &d_c)) || (rc = slot(c, S_RID, n, &d_rid)))
        return rc;
    hipLaunchKernelGGL(k_unpack_hit_rows, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, rows, (int64_t)60, d_ts, d_pos, d_s, d_e, d_dt,
                       d_b, d_c, d_rid);
    *h = HitCols{d_ts, d_pos, d_s, d_e, d_dt, d_b, d_c, d_rid};
    return WFA_OK;
}

// ---- event grouping ---------------------------------------------------------------------------------------
__global__ void k_gather_f64(int64_t n, const double* __restrict__ src, const int64_t* __restrict__ perm,
                             double* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) dst[i] = src[perm[i]];
}

// a hit opens a new event <=> its start lies more than `gap` after the latest end seen so far (:457-470)
__global__ void k_event_flags(int64_t n, const double* __restrict__ abs0, const int64_t* __restrict__ perm,
                              const double* __restrict__ run_max, double gap_ps, int64_t* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    flag[j] = (j == 0 || abs0[perm[j]] > run_max[j - 1] + gap_ps) ? 1 : 0;
}

__global__ void k_event_keys(int64_t n, const int64_t* __restrict__ perm, const int64_t* __restrict__ incl,
                             uint64_t* __restrict__ k_event) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j < n) k_event[perm[j]] = (uint64_t)(incl[j] - 1);
}

__global__ void k_event_starts(int64_t n, const uint64_t* __restrict__ k_event, const int64_t* __restrict__ perm,
                               int64_t n_events, int64_t* __restrict__ event_start) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    const uint64_t ev = k_event[perm[j]];
    if (j == 0 || k_event[perm[j - 1]] != ev) event_start[ev] = j;
    if (j == n - 1) event_start[n_events] = n;
}

__global__ void k_event_minmax(int64_t n_events, const int64_t* __restrict__ event_start,
                               const int64_t* __restrict__ perm, const double* __restrict__ abs0,
                               const double* __restrict__ abs1, int64_t* __restrict__ t_min,
                               int64_t* __restrict__ t_max, double* __restrict__ ev_hi) {
    const int64_t ev = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (ev >= n_events) return;
    const int64_t a = event_start[ev], b = event_start[ev + 1];
    double lo = abs0[perm[a]], hi = abs1[perm[a]];
    for (int64_t j = a + 1; j < b; ++j) {
        const double s = abs0[perm[j]], e = abs1[perm[j]];
        lo = s < lo ? s : lo;
        hi = e > hi ? e : hi;
    }
    t_min[ev] = (int64_t)lo;  // int(np.min(...)): truncation
    t_max[ev] = (int64_t)hi;
    if (ev_hi) ev_hi[ev] = hi;  // the event stream compares the untruncated end with its horizon
}

// The grouping pass over a device table of n > 0 hits (the body of wfa_group_hit_windows_count; the event stream runs it
// on carry ++ new rows): prep, lexsort, max-scan, flags, second sort, per-event tables.  Leaves, in scratch slots,
// abs_start / abs_end per hit (S_ABS0 / S_ABS1), the event index of every hit (S_K1), *perm = the hits event-major in the
// reference's order, event_start[n_ev + 1] (S_OUT0), t_min / t_max (S_OUT1 / S_OUT2) and, where ev_hi is given, the
// untruncated max(abs_end) per event.  ev_hi must hold n entries (n_ev <= n is known only inside).  The launches are
// queued on the context's stream; the last ones may still be running when this returns.
int group_cols(wfa_ctx* c, int64_t n, const HitCols& h, const double* fix0, const double* fix1, double time_window_ns,
               int64_t* n_events, int64_t** perm_out, double* ev_hi) {
    int rc;
    double *abs0, *abs1, *ends, *run_max;
    uint64_t *k_abs, *k_dt, *k_ts, *k_rid, *k_chan, *k_ev;
    int64_t *flag, *incl;
    if ((rc = slot(c, S_ABS0, n, &abs0)) || (rc = slot(c, S_ABS1, n, &abs1)) || (rc = slot(c, S_K0, n, &k_abs)) ||
        (rc = slot(c, S_K1, n, &k_dt)) || (rc = slot(c, S_K2, n, &k_ts)) || (rc = slot(c, S_K3, n, &k_rid)) ||
        (rc = slot(c, S_K4, n, &k_chan)) || (rc = slot(c, S_F0, n, &ends)) || (rc = slot(c, S_F1, n, &run_max)) ||
        (rc = slot(c, S_FLAG, n, &flag)) || (rc = slot(c, S_ID, n, &incl)))
        return rc;
    LaunchTimer t(c);
    if ((rc = hit_prep(c, n, h, fix0, fix1, abs0, abs1, k_abs, k_dt, k_ts, k_rid, k_chan))) return rc;
    int64_t* perm = nullptr;
    {
        const uint64_t* keys[4] = {k_abs, k_dt, k_ts, k_rid};  // np.lexsort((record_ids, timestamps, dt, abs_starts))
        if ((rc = lexsort(c, n, keys, 4, &perm))) return rc;
    }
    hipLaunchKernelGGL(k_gather_f64, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, abs1, perm, ends);
    size_t tb = 0;
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb, ends, run_max, (size_t)n, MaxF64(), c->stream));
    size_t tb2 = 0;
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb2, flag, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    if ((rc = c->ht[S_CUB].ensure(tb > tb2 ? tb : tb2))) return rc;
    tb = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, ends, run_max, (size_t)n, MaxF64(), c->stream));
    hipLaunchKernelGGL(k_event_flags, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, abs0, perm, run_max,
                       time_window_ns * 1e3, flag);
    tb = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, flag, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    int64_t n_ev = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&n_ev, incl + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    // event id as the new primary key; k_dt's buffer is free again (k_chan carries dt)
    k_ev = k_dt;
    hipLaunchKernelGGL(k_event_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, perm, incl, k_ev);
    {
        // np.lexsort((record_ids, timestamps, abs_starts, dt, channels, boards, event_id)).  The hits already stand in
        // (abs_start, dt, timestamp, record_id) order: a stable sort of THAT order by (event, board, channel, dt) leaves
        // every tie -- same event, channel and dt -- in (abs_start, timestamp, record_id) order, which is the reference's.
        // Two narrow keys instead of five (17 radix passes -> 4).
        const uint64_t* keys[2] = {k_ev, k_chan};
        if ((rc = lexsort(c, n, keys, 2, &perm, perm))) return rc;
    }
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    int64_t *ev_start, *t_min, *t_max;
    if ((rc = slot(c, S_OUT0, n_ev + 1, &ev_start)) || (rc = slot(c, S_OUT1, n_ev, &t_min)) || (rc = slot(c, S_OUT2, n_ev, &t_max)))
        return rc;
    hipLaunchKernelGGL(k_event_starts, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, k_ev, perm, n_ev, ev_start);
    hipLaunchKernelGGL(k_event_minmax, dim3(blocks_for(n_ev)), dim3(kTB), 0, c->stream, n_ev, ev_start, perm, abs0, abs1, t_min, t_max,
                       ev_hi);
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("hit table: group_hit_windows (sort + scans)"))) return rc;
    *n_events = n_ev;
    *perm_out = perm;
    return WFA_OK;
}

// ---- hit merge --------------------------------------------------------------------------------------------
// ---- legacy fixed-window grouping (group_multi_channel_hits, event_grouping.py:98-283, 475-525) ----------------------
// After a stable sort by timestamp a cluster takes every hit within `window` of its FIRST hit: the boundaries are the
// chain 0 -> next[0] -> next[next[0]] -> ... with next[i] = upper_bound(ts, ts[i] + window), compared in float64 like
// numpy's searchsorted of an int64 column against a float64 needle.  The chain is marked by pointer jumping, bottom up:
// with J_k = next^(2^k) and the marks {next^m(0) : m < 2^k} before level k, marking J_k of every marked hit gives
// {next^m(0) : m < 2^(k+1)}.  A level reads J_k and writes J_(k+1) in the same launch, so two (n+1)-entry levels are all
// the jump storage there is, whatever n; once J_k[0] == n every chain hit is marked and the later launches return at once.
__global__ void k_mc_keys(int64_t n, const int64_t* __restrict__ ts, const int64_t* __restrict__ ch,
                          uint64_t* __restrict__ k_ts, uint64_t* __restrict__ k_ch) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) { k_ts[i] = ord_i64(ts[i]); k_ch[i] = ord_i64(ch[i]); }
}
__global__ void k_mc_sorted_ts(int64_t n, const int64_t* __restrict__ ts, const int64_t* __restrict__ perm,
                               double* __restrict__ ts_f) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) ts_f[i] = (double)ts[perm[i]];
}
__global__ void k_mc_next(int64_t n, const double* __restrict__ ts_f, double window_ps, int32_t* __restrict__ nxt) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i > n) return;
    if (i == n) { nxt[n] = (int32_t)n; return; }
    const double needle = ts_f[i] + window_ps;
    int64_t lo = i + 1, hi = n;  // ts_f[i] <= needle (window >= 0, or NaN: then nothing is <= needle and the cluster is the hit alone)
    if (!(ts_f[i] <= needle)) { nxt[i] = (int32_t)(i + 1); return; }
    while (lo < hi) {  // first j in (i, n] with ts_f[j] > needle
        const int64_t mid = (lo + hi) >> 1;
        if (ts_f[mid] <= needle) lo = mid + 1; else hi = mid;
    }
    nxt[i] = (int32_t)lo;
}
__global__ void k_mc_mark_jump(int64_t n, const int32_t* __restrict__ j_in, int32_t* __restrict__ j_out,
                               int64_t* __restrict__ mark) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i > n) return;
    if (j_in[0] == n) {  // the chain from hit 0 ends within 2^k steps: marked already; pass the end on to the next level
        if (i == 0) j_out[0] = (int32_t)n;
        return;
    }
    const int32_t t = j_in[i];  // <= n, and j_in[n] == n
    j_out[i] = j_in[t];
    if (i < n && t < n && mark[i]) mark[t] = 1;  // (a mark set during this launch is a chain hit as well)
}
__global__ void k_mc_bounds(int64_t n, const int64_t* __restrict__ mark, const int64_t* __restrict__ incl, int64_t n_events,
                            int64_t* __restrict__ bounds) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n && mark[i]) bounds[incl[i] - 1] = i;
    if (i == n - 1) bounds[n_events] = n;
}

__global__ void k_merge_gather(int64_t n, const int64_t* __restrict__ perm, const double* __restrict__ abs0,
                               const double* __restrict__ abs1, const int32_t* __restrict__ dt,
                               const uint64_t* __restrict__ k_chan, double* __restrict__ s0, double* __restrict__ s1,
                               int32_t* __restrict__ sdt, uint64_t* __restrict__ sg) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    const int64_t i = perm[j];
    s0[j] = abs0[i]; s1[j] = abs1[i]; sdt[j] = dt[i]; sg[j] = k_chan[i];
}

// Running maximum of abs_end inside a hardware channel (segmented inclusive max-scan): a hit whose start lies
// more than merge_gap after EVERY earlier end of its channel certainly opens a new cluster, because the current
// cluster's end is one of those ends.  Such certain breaks (and channel / dt changes) cut the table into
// segments that chain independently; the total-width cap, which makes the chain a sequential greedy
// segmentation, only ever acts inside a segment.
struct SegMax {
    double v;
    int32_t head;  // 1: a channel starts here
    int32_t pad;
};
struct SegMaxOp {
    __device__ SegMax operator()(const SegMax& a, const SegMax& b) const {
        SegMax r;
        r.head = a.head | b.head;
        r.v = b.head ? b.v : (b.v > a.v ? b.v : a.v);
        r.pad = 0;
        return r;
    }
};
__global__ void k_merge_segin(int64_t n, const double* __restrict__ s1, const uint64_t* __restrict__ sg,
                              SegMax* __restrict__ in) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    SegMax x;
    x.v = s1[j];
    x.head = (j == 0 || sg[j] != sg[j - 1]) ? 1 : 0;
    x.pad = 0;
    in[j] = x;
}

// the chain of hit_merge.py:151-179 over one segment per lane: every lane looks at its own sorted position and
// walks only if a segment starts there (no list of heads: a single atomic counter serialises at ~90 appends / us)
__global__ void k_merge_chain(int64_t n, const double* __restrict__ s0, const double* __restrict__ s1,
                              const int32_t* __restrict__ sdt, const uint64_t* __restrict__ sg,
                              const SegMax* __restrict__ run, int do_merge,
                              double gap_ps, double max_width_ps, int64_t* __restrict__ flag) {
    int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    const bool head = j == 0 || sg[j] != sg[j - 1] || !do_merge || sdt[j] != sdt[j - 1] ||
                      !(s0[j] - run[j - 1].v <= gap_ps);
    if (!head) return;
    const uint64_t grp = sg[j];
    double c_start = s0[j], c_end = s1[j];
    int32_t prev_dt = sdt[j];
    flag[j] = 1;
    for (++j; j < n && sg[j] == grp; ++j) {
        if (!do_merge || sdt[j] != prev_dt || !(s0[j] - run[j - 1].v <= gap_ps)) break;  // the next segment's head
        const double a = s0[j], e = s1[j];
        const double gap = a - c_end;
        const double next_end = e > c_end ? e : c_end;
        const double total = next_end - c_start;
        const bool same_dt = sdt[j] == prev_dt;
        if (do_merge && same_dt && gap <= gap_ps && total <= max_width_ps) {
            flag[j] = 0;
            c_end = next_end;
        } else {
            flag[j] = 1;
            c_start = a;
            c_end = e;
        }
        prev_dt = sdt[j];
    }
}

__global__ void k_cluster_offsets(int64_t n, const int64_t* __restrict__ flag, const int64_t* __restrict__ incl,
                                  int64_t n_clusters, int64_t* __restrict__ offset) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    if (flag[j]) offset[incl[j] - 1] = j;
    if (j == n - 1) offset[n_clusters] = n;
}

// _emit_cluster (hit_merge.py:256-322) for every cluster, or for the n_clusters clusters `list` names (results indexed
// like the list); singles are flagged and copied on the host, or by k_ms_rows
__global__ void k_merge_emit(int64_t n_clusters, const int64_t* __restrict__ offset, const int64_t* __restrict__ perm,
                             HitCols h, const float* __restrict__ height, const float* __restrict__ integral,
                             int64_t* __restrict__ anchor, float* __restrict__ out_h, float* __restrict__ out_int,
                             int32_t* __restrict__ out_s, int32_t* __restrict__ out_e, float* __restrict__ out_w,
                             const int64_t* __restrict__ list = nullptr) {
    __shared__ double s_pw[kPairwiseLevels][kTB];
    const int64_t r = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (r >= n_clusters) return;
    const int64_t cl = list ? list[r] : r;
    const int64_t a = offset[cl], b = offset[cl + 1];
    int64_t best = perm[a];
    double max_h = (double)height[best];
    for (int64_t j = a + 1; j < b; ++j) {
        const double v = (double)height[perm[j]];
        if (v > max_h) max_h = v;  // np.max
    }
    // anchor: the member with the maximum height; ties -> the smallest timestamp, first such member
    bool have = false;
    for (int64_t j = a; j < b; ++j) {
        const int64_t i = perm[j];
        if ((double)height[i] != max_h) continue;
        if (!have || h.ts[i] < h.ts[best]) { best = i; have = true; }
    }
    int32_t smin = h.s[perm[a]], emax = h.e[perm[a]];
    bool one_record = true;
    const int64_t rid0 = h.rid[perm[a]];
    for (int64_t j = a + 1; j < b; ++j) {
        const int64_t i = perm[j];
        smin = h.s[i] < smin ? h.s[i] : smin;
        emax = h.e[i] > emax ? h.e[i] : emax;
        one_record = one_record && h.rid[i] == rid0;
    }
    if (!one_record) { smin = -1; emax = -1; }
    double w = (double)emax - (double)smin;  // python ints; max(.., 0.0)
    w = w > 0.0 ? w : 0.0;
    if (smin < 0 || emax < 0) w = -1.0;
    const double total = np_pairwise_sum([&](int q) { return (double)integral[perm[a + q]]; }, 0, (int)(b - a),
                                         &s_pw[0][threadIdx.x], kTB);
    anchor[r] = best;
    out_h[r] = (float)max_h;
    out_int[r] = (float)total;
    out_s[r] = smin;
    out_e[r] = emax;
    out_w[r] = (float)w;
}

// ---- records builder: global order + pool packing (records_builder.py:115-120, 164-209, 869-945) --------------
__global__ void k_record_keys(int64_t n, const int64_t* __restrict__ ts, const int32_t* __restrict__ pid,
                              const int16_t* __restrict__ board, const int16_t* __restrict__ chan,
                              uint64_t* __restrict__ k_ts, uint64_t* __restrict__ k_pid, uint64_t* __restrict__ k_bc) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    k_ts[i] = ord_i64(ts[i]);
    k_pid[i] = (uint64_t)((uint32_t)pid[i] ^ 0x80000000u);
    k_bc[i] = ((uint64_t)(uint16_t)(board[i] ^ (int16_t)0x8000) << 16) | (uint64_t)(uint16_t)(chan[i] ^ (int16_t)0x8000);
}

// one workgroup per record; 16-byte moves when source and destination are co-aligned, 2-byte moves otherwise
__global__ __launch_bounds__(128) void k_pool_gather(int64_t n, const int64_t* __restrict__ src_off,
                                                     const int64_t* __restrict__ dst_off,
                                                     const int32_t* __restrict__ length,
                                                     const uint16_t* __restrict__ src, uint16_t* __restrict__ dst) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const int64_t so = src_off[r], d0 = dst_off[r];
    const int len = length[r];
    if (len <= 0) return;
    const uint16_t* s = src + so;
    uint16_t* d = dst + d0;
    if (((so | d0) & 7) == 0) {
        const int nv = len >> 3;
        const uint4* s4 = reinterpret_cast<const uint4*>(s);
        uint4* d4 = reinterpret_cast<uint4*>(d);
        for (int i = threadIdx.x; i < nv; i += 128) d4[i] = s4[i];
        for (int i = (nv << 3) + threadIdx.x; i < len; i += 128) d[i] = s[i];
    } else {
        for (int i = threadIdx.x; i < len; i += 128) d[i] = s[i];
    }
}


// ---- st_waveforms rows: numpy's packed create_record_dtype(L) layout written on the device ---------------------------
// (reference: processing/dtypes.py:36-64; waveforms.py:640-734 / :233-290 fill the same rows with a strided host pass)
// Output-stationary: a lane owns 16 bytes of the batch's byte stream, finds its (row, byte-in-row) with a reciprocal
// multiply, composes the eight halfwords (header bytes, or samples realigned from two aligned dwords by a funnel shift,
// zero past the row's length) and stores them with one dwordx4 store.  The stride 76 + 2L is even, so a lane's first
// byte is always even and every halfword lies in one field; stores never straddle a lane.
constexpr uint32_t kStHeader = 76;   // baseline 0, baseline_upstream 8, polarity 16 (8 UCS-4), timestamp 48,
                                     // record_id 56, dt 64, event_length 68, board 72, channel 74, wave 76
constexpr int kStBlock = 256;
constexpr int kStMaxPol = 8;

struct StPackArgs {
    const uint16_t* src;         // device samples (4-byte aligned base)
    const int64_t* src_off;      // per row, samples
    const int32_t* src_len;
    const double* baseline;
    const double* baseline_up;
    const int64_t* ts;
    const int64_t* rid;
    const int32_t* dt;
    const int32_t* ev_len;
    const int16_t* board;
    const int16_t* chan;
    const uint8_t* pol;          // index into pol_tab
    const uint32_t* pol_tab;     // kStMaxPol x 8 UCS-4 code points
    int64_t row0;                // first row of this batch
    int64_t n_rows;              // rows in this batch
    uint32_t n_chunks;           // 16-byte chunks of this batch (the buffer is padded to a whole chunk)
    uint32_t stride;             // bytes per row
    uint32_t magic;              // floor((2^32 - 1) / stride)
    int32_t L;
};

// halfword h (0..37) of row r's header
__device__ __forceinline__ uint32_t st_header_half(const StPackArgs& a, int64_t r, uint32_t h) {
    uint64_t v;
    uint32_t k;
    if (h < 4) { v = (uint64_t)__double_as_longlong(a.baseline[r]); k = h; }
    else if (h < 8) { v = (uint64_t)__double_as_longlong(a.baseline_up[r]); k = h - 4; }
    else if (h < 24) { v = a.pol_tab[a.pol[r] * 8 + ((h - 8) >> 1)]; k = (h - 8) & 1; }
    else if (h < 28) { v = (uint64_t)a.ts[r]; k = h - 24; }
    else if (h < 32) { v = (uint64_t)a.rid[r]; k = h - 28; }
    else if (h < 34) { v = (uint32_t)a.dt[r]; k = h - 32; }
    else if (h < 36) { v = (uint32_t)a.ev_len[r]; k = h - 34; }
    else if (h == 36) { v = (uint16_t)a.board[r]; k = 0; }
    else { v = (uint16_t)a.chan[r]; k = 0; }
    return (uint32_t)(v >> (16 * k)) & 0xffffu;
}

__device__ __forceinline__ int32_t st_len(const StPackArgs& a, int64_t r) {
    const int32_t n = a.src_len[r];
    return n <= 0 ? 0 : (n < a.L ? n : a.L);
}

__global__ __launch_bounds__(kStBlock) void k_st_pack(StPackArgs a, uint8_t* __restrict__ out) {
    const uint32_t g = blockIdx.x * kStBlock + threadIdx.x;
    if (g >= a.n_chunks) return;
    const uint32_t b = g * 16u;
    uint32_t r = __umulhi(b, a.magic);  // floor(b / stride) or up to two less
    uint32_t p = b - r * a.stride;
    if (p >= a.stride) { ++r; p -= a.stride; }
    if (p >= a.stride) { ++r; p -= a.stride; }
    uint32_t w[4];
    if (p >= kStHeader && p + 16 <= a.stride) {
        // eight samples of one row: s0 .. s0 + 7
        const int64_t gr = a.row0 + r;
        const int64_t off = a.src_off[gr];
        const int32_t len = st_len(a, gr);
        const int32_t s0 = (int32_t)((p - kStHeader) >> 1);
        const int64_t at = off + s0, lim = off + len;   // sample indices into src; [.., lim) is this row's to write
        const int64_t ab = at >> 1;
        const bool odd = at & 1;
        const uint32_t* src32 = reinterpret_cast<const uint32_t*>(a.src);
        const bool any = s0 < len;   // (a row of length 0 may carry any offset: nothing of it is read)
        uint32_t d[5];
#pragma unroll
        for (int i = 0; i < 5; ++i)  // only dwords holding a sample of this row are read
            d[i] = (any && (i < 4 || odd) && 2 * (ab + i) < lim) ? src32[ab + i] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t v = odd ? __builtin_amdgcn_alignbit(d[j + 1], d[j], 16) : d[j];
            const int32_t s = s0 + 2 * j;
            if (s >= len) v = 0;
            else if (s + 1 >= len) v &= 0xffffu;
            w[j] = v;
        }
    } else {
        // header bytes, a row boundary or the padding after the last row: halfword by halfword
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                uint32_t q = p + 4 * j + 2 * k;
                uint32_t rr = r;
                if (q >= a.stride) { q -= a.stride; ++rr; }
                uint32_t hw = 0;
                if (rr < a.n_rows) {
                    const int64_t gr = a.row0 + rr;
                    if (q < kStHeader) {
                        hw = st_header_half(a, gr, q >> 1);
                    } else {
                        const int32_t s = (int32_t)((q - kStHeader) >> 1);
                        if (s < st_len(a, gr)) hw = a.src[a.src_off[gr] + s];
                    }
                }
                v |= hw << (16 * k);
            }
            w[j] = v;
        }
    }
    *reinterpret_cast<uint4*>(out + b) = make_uint4(w[0], w[1], w[2], w[3]);
}


// ---- K15: delimiter-separated integer text -> int64 columns + uint16 samples (CAEN VX2730 CSV) ------------------
// (utils/formats/vx2730.py:193-340: every reader backend yields the same integers; records_builder.py:212-302 then
// uses columns board / channel / timestamp and the samples from `samples_start` to the end of the row.)
// A row is the bytes between two '\n' (a trailing '\r' dropped); an empty row has 0 fields.  One wave decodes one
// row in 1-KiB tiles: the tile (+ 32 bytes of lookahead) is staged in LDS with 16-byte loads, every lane counts the
// delimiters of its 16 bytes, a wave prefix sum turns that into the field index, and the lane parses the fields that
// FOLLOW its delimiters (a decimal integer is at most 20 characters, so the lookahead always covers it).
constexpr int kCsvTile = 1024;
constexpr int kCsvLook = 32;
constexpr int kCsvMaxMeta = 8;
constexpr int kCsvErrSyntax = 1, kCsvErrRange = 2;

// newline positions in text order: a thread owns 16 bytes; pass 1 counts per block, pass 2 (after a scan of the block
// counts) writes the positions.  (A DeviceSelect over one item per byte took 3.3 ms per 150 MB; this takes 0.1 ms.)
constexpr int kCsvNlBlock = 256;

template <bool FILL>
__global__ __launch_bounds__(kCsvNlBlock) void k_csv_newlines(int64_t n_bytes, const uint8_t* __restrict__ text,
                                                             const int64_t* __restrict__ block_start,
                                                             int64_t* __restrict__ block_count, int64_t* __restrict__ nl) {
    using Scan = rocprim::block_scan<int, kCsvNlBlock>;
    __shared__ typename Scan::storage_type tmp;
    const int64_t a = ((int64_t)blockIdx.x * kCsvNlBlock + threadIdx.x) * 16;
    uint32_t m = 0;
    if (a < n_bytes) {  // the buffer is padded, the clip drops the padding
        const uint4 w = *reinterpret_cast<const uint4*>(text + a);
        const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) m |= (uint32_t)(((v[k >> 2] >> ((k & 3) * 8)) & 0xffu) == '\n') << k;
        if (a + 16 > n_bytes) m &= (1u << (int)(n_bytes - a)) - 1u;
    }
    int before = 0, total = 0;
    Scan().exclusive_scan(__popc(m), before, 0, total, tmp, rocprim::plus<int>());
    if (!FILL) {
        if (threadIdx.x == 0) block_count[blockIdx.x] = total;
        return;
    }
    int64_t o = block_start[blockIdx.x] + before;
    while (m) {
        nl[o++] = a + (__ffs(m) - 1);
        m &= m - 1;
    }
}

__global__ void k_csv_lines(int64_t n_lines, int64_t n_nl, int64_t n_bytes, const uint8_t* __restrict__ text,
                            const int64_t* __restrict__ nl, int64_t* __restrict__ row_start, int64_t* __restrict__ row_end) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n_lines) return;
    const int64_t s = i == 0 ? 0 : nl[i - 1] + 1;
    int64_t e = i < n_nl ? nl[i] : n_bytes;
    if (e > s && text[e - 1] == '\r') --e;
    row_start[i] = s;
    row_end[i] = e;
}

__device__ __forceinline__ uint32_t csv_delim_mask(const uint4& w, uint8_t delim) {
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) m |= (uint32_t)(((v[k >> 2] >> ((k & 3) * 8)) & 0xffu) == delim) << k;
    return m;
}

// restrict a 16-bit byte mask of the chunk at absolute offset `abs0` to the bytes in [lo, hi)
__device__ __forceinline__ uint32_t csv_clip(uint32_t m, int64_t abs0, int64_t lo, int64_t hi) {
    if (abs0 + 16 <= lo || abs0 >= hi) return 0;
    if (abs0 < lo) m &= ~0u << (int)(lo - abs0);
    if (abs0 + 16 > hi) m &= (1u << (int)(hi - abs0)) - 1u;
    return m;
}

// fields per row and samples per row (fields from samples_start on); one wave per row
__global__ __launch_bounds__(64) void k_csv_count(int64_t n_rows, const uint8_t* __restrict__ text,
                                                  const int64_t* __restrict__ row_start, const int64_t* __restrict__ row_end,
                                                  uint8_t delim, int32_t samples_start, int32_t* __restrict__ n_fields,
                                                  int64_t* __restrict__ n_samples) {
    const int64_t r = blockIdx.x;
    if (r >= n_rows) return;
    const int lane = threadIdx.x;
    const int64_t lo = row_start[r], hi = row_end[r];
    int cnt = 0;
    for (int64_t a = (lo & ~15ll) + lane * 16; a < hi; a += 64 * 16) {
        const uint4 w = *reinterpret_cast<const uint4*>(text + a);
        cnt += __popc(csv_clip(csv_delim_mask(w, delim), a, lo, hi));
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) {
        const int nf = hi > lo ? cnt + 1 : 0;
        n_fields[r] = nf;
        n_samples[r] = nf > samples_start ? nf - samples_start : 0;
    }
}

struct CsvCols {
    int32_t n_meta;
    int32_t col[kCsvMaxMeta];
};

__global__ __launch_bounds__(64) void k_csv_decode(int64_t n_rows, const uint8_t* __restrict__ text,
                                                   const int64_t* __restrict__ row_start, const int64_t* __restrict__ row_end,
                                                   uint8_t delim, int32_t samples_start, CsvCols cols,
                                                   const int64_t* __restrict__ sample_offset, int64_t* __restrict__ meta,
                                                   uint16_t* __restrict__ samples, unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[kCsvTile + kCsvLook];
    const int64_t r = blockIdx.x;
    if (r >= n_rows) return;
    const int lane = threadIdx.x;
    const int64_t lo = row_start[r], hi = row_end[r];
    if (hi <= lo) return;
    const int64_t s_off = sample_offset[r];
    int field_base = 0;  // delimiters of the row before this tile
    for (int64_t t0 = lo & ~15ll; t0 < hi; t0 += kCsvTile) {
        __syncthreads();
        const uint4 w = *reinterpret_cast<const uint4*>(text + t0 + lane * 16);
        *reinterpret_cast<uint4*>(tile + lane * 16) = w;
        if (lane < kCsvLook / 16)
            *reinterpret_cast<uint4*>(tile + kCsvTile + lane * 16) =
                *reinterpret_cast<const uint4*>(text + t0 + kCsvTile + lane * 16);
        __syncthreads();
        const int64_t a = t0 + lane * 16;
        uint32_t m = csv_clip(csv_delim_mask(w, delim), a, lo, hi);
        const int mine = __popc(m);
        int incl = mine;  // inclusive prefix over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        int f = field_base + incl - mine;  // index of the field that CONTAINS this lane's first byte
        // the lane owning the row's first byte also parses field 0 (a virtual delimiter before the row)
        bool first = lo >= a && lo < a + 16;
        while (first || m) {
            int64_t q;  // absolute offset of the field's first character
            if (first) { q = lo; first = false; }
            else { const int b = __ffs(m) - 1; m &= m - 1; q = a + b + 1; ++f; }
            const int fidx = (q == lo) ? 0 : f;
            bool is_meta = false;  // (a column may be requested more than once: every request is filled)
            for (int j = 0; j < cols.n_meta; ++j) is_meta |= cols.col[j] == fidx;
            const bool is_sample = fidx >= samples_start;
            if (!is_meta && !is_sample) continue;
            int p = (int)(q - t0);
            const int p_end = (int)((hi - t0) < (int64_t)(kCsvTile + kCsvLook) ? (hi - t0) : (kCsvTile + kCsvLook));
            bool neg = false, any = false, bad = false;
            unsigned long long v = 0;
            if (p < p_end && (tile[p] == '-' || tile[p] == '+')) { neg = tile[p] == '-'; ++p; }
            int digits = 0;
            for (; p < p_end; ++p) {
                const uint8_t ch = tile[p];
                if (ch == delim) break;
                if (ch < '0' || ch > '9' || ++digits > 19) { bad = true; break; }
                v = v * 10ull + (unsigned long long)(ch - '0');
                any = true;
            }
            if (!any || bad || v > 0x7fffffffffffffffull) {
                atomicMin(err, ((unsigned long long)r << 24) | ((unsigned long long)(fidx & 0x3fffff) << 2) | kCsvErrSyntax);
                continue;
            }
            const int64_t val = neg ? -(int64_t)v : (int64_t)v;
            for (int j = 0; j < cols.n_meta; ++j)
                if (cols.col[j] == fidx) meta[r * cols.n_meta + j] = val;
            if (is_sample) {
                if (val < 0 || val > 65535)
                    atomicMin(err, ((unsigned long long)r << 24) | ((unsigned long long)(fidx & 0x3fffff) << 2) | kCsvErrRange);
                else
                    samples[s_off + (fidx - samples_start)] = (uint16_t)val;
            }
        }
        int total = __shfl(incl, 63);
        field_base += total;
    }
}

// ---- event stream (wfa_event_stream_*) -----------------------------------------------------------------------------
// A push groups carry ++ new rows with group_cols, closes the events that end more than the window before the horizon
// (a prefix of the table's events: no later hit can join or precede them), writes their hits as 84-byte rows and keeps
// the hits of the open events, in their original row order, for the next push.
constexpr int kEsBadDt = 1, kEsBadEdge = 2;
struct EsCtl {
    unsigned long long min_key;   // ord_f64 of the smallest abs_start among the pushed rows
    unsigned long long n_closed;  // events of the closed prefix (starts at n_events, lowered to the first open event)
    long long n_out;              // hits of the closed prefix
    int flags, pad;
};

// the pushed rows [0, n) (columns and windows already offset past the carry): dt and edge checks, smallest abs_start;
// Ctl = the control block of the event stream or of the merge stream
template <typename Ctl>
__global__ __launch_bounds__(kTB) void k_es_check(int64_t n, const int32_t* __restrict__ dt, const int32_t* __restrict__ s,
                                                  const int32_t* __restrict__ e, const double* __restrict__ abs0,
                                                  Ctl* __restrict__ ctl) {
    unsigned long long lo = ~0ull;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x; i < n; i += (int64_t)gridDim.x * kTB) {
        if (dt[i] <= 0) bad |= kEsBadDt;
        if (s[i] < 0 || e[i] < 0) bad |= kEsBadEdge;
        const unsigned long long k = ord_f64(abs0[i]);
        lo = k < lo ? k : lo;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, d);
        lo = ol < lo ? ol : lo;
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin(&ctl->min_key, lo);
        if (bad) atomicOr(&ctl->flags, bad);
    }
}

// closed <=> max(abs_end) + gap < horizon, strictly; the first open event bounds the prefix
__global__ void k_es_closed(int64_t n_events, const double* __restrict__ ev_hi, double gap_ps, double horizon,
                            EsCtl* __restrict__ ctl) {
    const int64_t ev = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (ev >= n_events) return;
    if (ev_hi[ev] + gap_ps < horizon) return;
    if (ev > 0 && !(ev_hi[ev - 1] + gap_ps < horizon)) return;  // not the first of its run of open events
    atomicMin(&ctl->n_closed, (unsigned long long)ev);
}
__global__ void k_es_count(const int64_t* __restrict__ event_start, EsCtl* __restrict__ ctl) {
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->n_out = event_start[ctl->n_closed];
}

// 84-byte rows as 21 dwords: event_id, t_min, t_max (6 dwords), then the hit's 15 dwords; lanes over dwords.  In general
// the first W dwords of table entries of S dwords (W = 18, S = 22: a 72-byte merged row out of an 88-byte entry, 96-byte rows)
template <int W, int S>
__global__ __launch_bounds__(kTB) void k_es_rows(int64_t n_out, const int64_t* __restrict__ perm,
                                                 const uint64_t* __restrict__ k_event, const int64_t* __restrict__ t_min,
                                                 const int64_t* __restrict__ t_max, int64_t first_event,
                                                 const uint32_t* __restrict__ rows, uint32_t* __restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (d >= n_out * (6 + W)) return;
    const int64_t j = d / (6 + W);
    const int w = (int)(d - j * (6 + W));
    const int64_t i = perm[j];
    if (w >= 6) { out[d] = rows[i * S + (w - 6)]; return; }
    const int64_t ev = (int64_t)k_event[i];
    const int64_t v = w < 2 ? first_event + ev : (w < 4 ? t_min[ev] : t_max[ev]);
    out[d] = (w & 1) ? (uint32_t)((uint64_t)v >> 32) : (uint32_t)(uint64_t)v;
}

__global__ void k_es_keep(int64_t n, const uint64_t* __restrict__ k_event, int64_t n_closed, int64_t* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) flag[i] = (int64_t)k_event[i] >= n_closed ? 1 : 0;
}
// the kept rows, W dwords each (15: a 60-byte hit row), to their place in the other carry buffer (original row order)
template <int W>
__global__ __launch_bounds__(kTB) void k_es_compact(int64_t n, const int64_t* __restrict__ flag,
                                                    const int64_t* __restrict__ incl, const uint32_t* __restrict__ src,
                                                    uint32_t* __restrict__ dst) {
    const int64_t d = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (d >= n * W) return;
    const int64_t i = d / W;
    if (flag[i]) dst[(incl[i] - 1) * W + (d - i * W)] = src[d];
}

// grow a carry buffer to `want` bytes and keep its first `used` bytes (DevBuf::ensure drops the contents)
int es_grow(wfa_ctx* c, DevBuf& b, size_t used, size_t want) {
    if (want <= b.cap) return WFA_OK;
    if (used == 0) return b.ensure(want);
    if (want < 2 * b.cap) want = 2 * b.cap;
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want + 256);
    if (e != hipSuccess) return fail(WFA_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    e = hipMemcpyAsync(p, b.ptr, used, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(WFA_E_HIP, "growing a stream's carry failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(b.ptr);
    b.ptr = p;
    b.cap = want;
    return WFA_OK;
}

}  // namespace

int Carry::reserve(wfa_ctx* c, int64_t n_new) { return es_grow(c, table(), (size_t)n * row, (size_t)(n + n_new) * row); }

// (a refused push leaves its rows there: they lie behind n and the next push overwrites them)
int Carry::upload(wfa_ctx* c, const void* rows, int64_t n_new) {
    return n_new > 0 ? h2d_copy(c, table().as<uint8_t>() + (size_t)n * row, rows, (size_t)n_new * row) : WFA_OK;
}

int Carry::compact(wfa_ctx* c, int64_t n_table, const int64_t* flag, const int64_t* incl, int64_t n_keep) {
    DevBuf& other = buf[cur ^ 1];
    const int rc = other.ensure((size_t)n_keep * row);
    if (rc) return rc;
    const int words = row / 4;
    const dim3 grid(blocks_for(n_table * words));
    const uint32_t* src = table().as<uint32_t>();
    uint32_t* dst = other.as<uint32_t>();
    switch (words) {
    case 2: hipLaunchKernelGGL(k_es_compact<2>, grid, dim3(kTB), 0, c->stream, n_table, flag, incl, src, dst); break;
    case 10: hipLaunchKernelGGL(k_es_compact<10>, grid, dim3(kTB), 0, c->stream, n_table, flag, incl, src, dst); break;
    case 15: hipLaunchKernelGGL(k_es_compact<15>, grid, dim3(kTB), 0, c->stream, n_table, flag, incl, src, dst); break;
    case 22: hipLaunchKernelGGL(k_es_compact<22>, grid, dim3(kTB), 0, c->stream, n_table, flag, incl, src, dst); break;
    default: return fail(WFA_E_INVALID, "no carry of %d-byte rows", row);
    }
    return WFA_OK;
}

namespace {

inline uint64_t host_ord_f64(double v) {
    uint64_t b;
    memcpy(&b, &v, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// The merge pass over a device table of n > 0 hits (the body of wfa_hit_merge_count; the merge stream runs it on
// carry ++ new rows): prep, sort per hardware channel, segmented max-scan, greedy chain, cluster offsets.  Leaves, in
// scratch slots, abs_start / abs_end per hit (S_ABS0 / S_ABS1), the sorted columns s0 / s1 / dt / channel key (S_F0 / S_F1 /
// S_K1 / S_SG), the head flag of every sorted position and its inclusive scan = cluster index + 1 (S_FLAG / S_ID),
// cluster_offset[n_clusters + 1] (S_OUT0) and *perm_out = the hits channel-major in chain order.  The launches are queued
// on the context's stream; the last one may still be running when this returns.
int merge_cols(wfa_ctx* c, int64_t n, const HitCols& h, double merge_gap_ns, double max_total_width_ns, int64_t* n_clusters,
               int64_t** perm_out) {
    int rc;
    double *abs0, *abs1, *s0, *s1;
    uint64_t *k_abs, *k_chan, *sg;
    int32_t* sdt;
    int64_t *flag, *incl;
    if ((rc = slot(c, S_ABS0, n, &abs0)) || (rc = slot(c, S_ABS1, n, &abs1)) || (rc = slot(c, S_K0, n, &k_abs)) ||
        (rc = slot(c, S_K4, n, &k_chan)) || (rc = slot(c, S_F0, n, &s0)) || (rc = slot(c, S_F1, n, &s1)) ||
        (rc = slot(c, S_K1, n, &sdt)) || (rc = slot(c, S_SG, n, &sg)) || (rc = slot(c, S_FLAG, n, &flag)) ||
        (rc = slot(c, S_ID, n, &incl)))
        return rc;
    LaunchTimer t(c);
    if ((rc = hit_prep(c, n, h, nullptr, nullptr, abs0, abs1, k_abs, nullptr, nullptr, nullptr, k_chan))) return rc;
    int64_t* perm = nullptr;
    {
        // per hardware channel (ascending board, channel), stable by abs_start (hit_merge.py:137-149)
        const uint64_t* keys[2] = {k_chan, k_abs};
        if ((rc = lexsort(c, n, keys, 2, &perm))) return rc;
    }
    hipLaunchKernelGGL(k_merge_gather, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, perm, abs0, abs1, h.dt, k_chan, s0, s1, sdt, sg);
    SegMax *seg_in, *seg_run;
    if ((rc = slot(c, S_OUT1, n, &seg_in)) || (rc = slot(c, S_OUT2, n, &seg_run))) return rc;
    const int do_merge = merge_gap_ns > 0 ? 1 : 0;
    const double gap_ps = merge_gap_ns * 1e3;
    hipLaunchKernelGGL(k_merge_segin, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, s1, sg, seg_in);
    size_t tb = 0, tb_seg = 0;
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb_seg, seg_in, seg_run, (size_t)n, SegMaxOp(), c->stream));
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb, flag, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    if ((rc = c->ht[S_CUB].ensure(tb > tb_seg ? tb : tb_seg))) return rc;
    tb_seg = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb_seg, seg_in, seg_run, (size_t)n, SegMaxOp(), c->stream));
    hipLaunchKernelGGL(k_merge_chain, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, s0, s1, sdt, sg, seg_run, do_merge,
                       gap_ps, max_total_width_ns * 1e3, flag);
    tb = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, flag, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    int64_t n_cl = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&n_cl, incl + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    int64_t* offset;
    if ((rc = slot(c, S_OUT0, n_cl + 1, &offset))) return rc;
    hipLaunchKernelGGL(k_cluster_offsets, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, flag, incl, n_cl, offset);
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("hit table: hit_merge clusters (sort + chain)"))) return rc;
    *n_clusters = n_cl;
    *perm_out = perm;
    return WFA_OK;
}


// ---- merge stream (wfa_merge_stream_*) ------------------------------------------------------------------------------
// A push chains carry ++ new rows with merge_cols and closes, per hardware channel, the clusters no later hit can precede
// or join.  With F = the rows of the channel that start below the horizon H, strictly, a cluster at sorted positions
// [a, b) is closed iff b <= F and (b < F, or nothing merges, or H - cluster_end > gap): a prefix of the channel's clusters.
// Their merged rows and member indices go out; the hits of all other clusters stay, in original row order, for the next push.
struct MsCtl {
    unsigned long long min_key;   // ord_f64 of the smallest abs_start among the pushed rows
    unsigned long long open_key;  // ord_f64 of the smallest abs_start among the rows that stay carried; ~0: none stay
    long long n_closed;           // closed clusters
    long long n_comp;             // their members
    int flags, pad;
};

// the pushed rows' indices in the sequence of all rows pushed since _begin
__global__ void k_ms_number(int64_t n, int64_t base, int64_t* __restrict__ index) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i < n) index[i] = base + i;
}

// height / integral columns of 60-byte rows (dwords 2 and 3) for k_merge_emit
__global__ void k_ms_cols(int64_t n, const uint32_t* __restrict__ rows, float* __restrict__ height,
                          float* __restrict__ integral) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    height[i] = __uint_as_float(rows[i * 15 + 2]);
    integral[i] = __uint_as_float(rows[i * 15 + 3]);
}

// closed flag and member count (0 for an open cluster) per cluster.  s0 ascends inside a channel, so b <= F is
// s0[b - 1] < H and b < F is "the next row belongs to the channel and starts below H"; cluster_end = max(abs_end).
__global__ void k_ms_closed(int64_t n_clusters, int64_t n, const int64_t* __restrict__ offset, const double* __restrict__ s0,
                            const double* __restrict__ s1, const uint64_t* __restrict__ sg, int do_merge, double gap_ps,
                            double horizon, int64_t* __restrict__ closed, int64_t* __restrict__ count) {
    const int64_t cl = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (cl >= n_clusters) return;
    const int64_t a = offset[cl], b = offset[cl + 1];
    bool done = s0[b - 1] < horizon;
    if (done && do_merge && !(b < n && sg[b] == sg[a] && s0[b] < horizon)) {
        double c_end = s1[a];
        for (int64_t j = a + 1; j < b; ++j) c_end = s1[j] > c_end ? s1[j] : c_end;
        done = horizon - c_end > gap_ps;
    }
    closed[cl] = done ? 1 : 0;
    count[cl] = done ? b - a : 0;
}

// keep flag per table row (1: its cluster stays open), the smallest abs_start among the kept rows, and, from one lane,
// the totals of the two scans
__global__ __launch_bounds__(kTB) void k_ms_keep(int64_t n, int64_t n_clusters, const int64_t* __restrict__ perm,
                                                 const int64_t* __restrict__ cluster_incl, const int64_t* __restrict__ closed,
                                                 const int64_t* __restrict__ closed_incl, const int64_t* __restrict__ comp_incl,
                                                 const double* __restrict__ s0, int64_t* __restrict__ keep,
                                                 MsCtl* __restrict__ ctl) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    unsigned long long lo = ~0ull;
    if (j < n) {
        const bool open = !closed[cluster_incl[j] - 1];
        keep[perm[j]] = open ? 1 : 0;
        if (open) lo = ord_f64(s0[j]);
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, d);
        lo = ol < lo ? ol : lo;
    }
    if ((threadIdx.x & 63) == 0 && lo != ~0ull) atomicMin(&ctl->open_key, lo);
    if (j == 0) {
        ctl->n_closed = closed_incl[n_clusters - 1];
        ctl->n_comp = comp_incl[n_clusters - 1];
    }
}

// list[r] = the r-th closed cluster
__global__ void k_ms_list(int64_t n_clusters, const int64_t* __restrict__ closed, const int64_t* __restrict__ closed_incl,
                          int64_t* __restrict__ list) {
    const int64_t cl = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (cl < n_clusters && closed[cl]) list[closed_incl[cl] - 1] = cl;
}

// 72-byte HIT_MERGED_DTYPE rows as 18 dwords, lanes over dwords: the anchor hit's 15 dwords with height, integral,
// sample_start, sample_end, width (dwords 2..6) replaced by the cluster's reductions -- a cluster of one hit keeps the
// hit's own (hit_merge.py:266-284) -- then component_offset (i8) and component_count (i4).  Row r goes to out + r * out_words
// (18: packed rows; 22: the merged-event stream's carry entries, whose last 4 dwords k_mes_fix writes)
__global__ __launch_bounds__(kTB) void k_ms_rows(int64_t n_out, const int64_t* __restrict__ list,
                                                 const int64_t* __restrict__ offset, const int64_t* __restrict__ comp_incl,
                                                 int64_t first_component, const int64_t* __restrict__ anchor,
                                                 const float* __restrict__ red_h, const float* __restrict__ red_int,
                                                 const int32_t* __restrict__ red_s, const int32_t* __restrict__ red_e,
                                                 const float* __restrict__ red_w, const uint32_t* __restrict__ rows,
                                                 uint32_t* __restrict__ out, int out_words) {
    const int64_t d = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (d >= n_out * 18) return;
    const int64_t r = d / 18;
    const int w = (int)(d - r * 18);
    const int64_t cl = list[r];
    const int64_t count = offset[cl + 1] - offset[cl];
    uint32_t v;
    if (w >= 15) {
        const int64_t first = first_component + comp_incl[cl] - count;
        v = w == 15 ? (uint32_t)(uint64_t)first : (w == 16 ? (uint32_t)((uint64_t)first >> 32) : (uint32_t)count);
    } else if (count == 1 || w < 2 || w > 6) {
        v = rows[anchor[r] * 15 + w];
    } else {
        v = w == 2 ? __float_as_uint(red_h[r]) : w == 3 ? __float_as_uint(red_int[r]) : w == 4 ? (uint32_t)red_s[r]
          : w == 5 ? (uint32_t)red_e[r] : __float_as_uint(red_w[r]);
    }
    out[r * out_words + w] = v;
}

// abs_start_fix / abs_end_fix of the closed clusters (event_grouping.py:369-416) into dwords 18..21 of their 22-dword
// entries: where the merged row has no sample window (its cluster spans records: -1, -1) the extent of the member hits,
// min abs_start and max abs_end over the sorted positions [a, b); NaN for every other cluster (the anchor formula holds)
__global__ void k_mes_fix(int64_t n_out, const int64_t* __restrict__ list, const int64_t* __restrict__ offset,
                          const double* __restrict__ s0, const double* __restrict__ s1, const int32_t* __restrict__ red_s,
                          const int32_t* __restrict__ red_e, double* __restrict__ entries) {
    const int64_t r = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (r >= n_out) return;
    double lo = __longlong_as_double(0x7ff8000000000000ll), hi = lo;
    if (red_s[r] < 0 || red_e[r] < 0) {
        const int64_t cl = list[r];
        const int64_t a = offset[cl], b = offset[cl + 1];
        lo = s0[a]; hi = s1[a];
        for (int64_t j = a + 1; j < b; ++j) {
            lo = s0[j] < lo ? s0[j] : lo;
            hi = s1[j] > hi ? s1[j] : hi;
        }
    }
    entries[r * 11 + 9] = lo;
    entries[r * 11 + 10] = hi;
}
// ... and back out of the n entries of a table as the two columns group_cols takes
__global__ void k_mes_fixcols(int64_t n, const double* __restrict__ entries, double* __restrict__ fix0,
                              double* __restrict__ fix1) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    fix0[i] = entries[i * 11 + 9];
    fix1[i] = entries[i * 11 + 10];
}

// hit_index of the closed clusters' members: clusters in the order of the merged rows, members in chain order
__global__ void k_ms_members(int64_t n, const int64_t* __restrict__ perm, const int64_t* __restrict__ cluster_incl,
                             const int64_t* __restrict__ closed, const int64_t* __restrict__ offset,
                             const int64_t* __restrict__ comp_incl, const int64_t* __restrict__ index,
                             int64_t* __restrict__ hit_index) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j >= n) return;
    const int64_t cl = cluster_incl[j] - 1;
    if (!closed[cl]) return;
    const int64_t a = offset[cl];
    hit_index[comp_incl[cl] - (offset[cl + 1] - a) + (j - a)] = index[perm[j]];
}

inline double host_unord_f64(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    double v;
    memcpy(&v, &b, sizeof(v));
    return v;
}

int plus_scan(wfa_ctx* c, const int64_t* in, int64_t* out, int64_t n) {
    int rc;
    size_t tb = 0;
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb, in, out, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    if ((rc = c->ht[S_CUB].ensure(tb))) return rc;
    tb = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, in, out, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    return WFA_OK;
}

// ---- the two steps of a push ----------------------------------------------------------------------------------------
// wfa_merge_stream_push is the merge step on c->ms, wfa_event_stream_push the group step on c->es; a push of the
// merged-event stream is one after the other on a state of its own, the merged rows handed over in HBM.  A step reads its
// stream's counters and changes none of them -- it only fills buffers behind what the carries hold: what it decides comes
// back in *r and the caller commits (merge_commit / group_commit) once the whole push has succeeded, so a refused push
// leaves every carry as it was.

// The checks every push makes before it touches the device: stream open, argument pointers, horizon not NaN and not below
// the previous push's, carry + pushed rows below 2^31.  The output of the previous push is void from here on (*out_count =
// -1): a push that is refused leaves nothing to fill.  H: double (ps) or int64_t (the df_events stream's timestamps)
inline bool horizon_nan(double h) { return h != h; }
inline bool horizon_nan(int64_t) { return false; }
inline int horizon_below(double h, double prev) {
    return fail(WFA_E_INVALID, "the horizon (%.17g ps) lies below the previous push's (%.17g ps)", h, prev);
}
inline int horizon_below(int64_t h, int64_t prev) {
    return fail(WFA_E_INVALID, "the horizon (%lld ps) lies below the previous push's (%lld ps)", (long long)h, (long long)prev);
}
template <typename H>
int push_checks(bool open, const char* what, const char* begin, int64_t* out_count, bool args_ok, H horizon, H previous,
                int64_t n_carry, int64_t n_rows) {
    if (!open) return fail(WFA_E_STATE, "no %s stream is open (%s first)", what, begin);
    *out_count = -1;
    if (!args_ok) return fail(WFA_E_INVALID, "bad arguments");
    if (horizon_nan(horizon)) return fail(WFA_E_INVALID, "the horizon is NaN");
    if (horizon < previous) return horizon_below(horizon, previous);
    if (n_rows >= 0x80000000LL - n_carry)
        return fail(WFA_E_INVALID, "carry (%lld rows) + pushed rows (%lld) reach the table limit of 2^31 rows",
                    (long long)n_carry, (long long)n_rows);
    return WFA_OK;
}

// where the merge step's merged rows go: n_closed entries of out_words dwords behind the first out_used entries of `out`,
// which are kept
struct MergeIo {
    DevBuf* out;
    int out_words;      // 18: HIT_MERGED_DTYPE rows; 22: with the fix windows behind each row (k_mes_fix)
    int64_t out_used;
};
struct MergeStepOut {
    int64_t n_closed = 0, n_comp = 0, n_keep = 0;
    double open_start = HUGE_VAL;
    bool flip = false;  // the carries went to their other buffers
};

int merge_step(wfa_ctx* c, wfa_ctx::MergeStream& ms, const MergeIo& io, const void* hit_rows, int64_t n_rows,
               double horizon_ps, MergeStepOut* r) {
    int rc;
    *r = MergeStepOut{};
    const int64_t n_carry = ms.carry.n, n = n_carry + n_rows;
    if (n == 0) return WFA_OK;  // nothing carried, nothing pushed: no launch
    c->ht_n = -1;  // the scratch slots a static count pass left for its fill are overwritten
    if ((rc = ms.carry.reserve(c, n_rows)) || (rc = ms.index.reserve(c, n_rows))) return rc;
    uint8_t* rows = ms.carry.table().as<uint8_t>();
    int64_t* index = ms.index.table().as<int64_t>();
    // 1. the pushed rows and their indices behind the carry
    if (n_rows > 0) {
        if ((rc = ms.carry.upload(c, hit_rows, n_rows))) return rc;
        hipLaunchKernelGGL(k_ms_number, dim3(blocks_for(n_rows)), dim3(kTB), 0, c->stream, n_rows, ms.next_hit, index + n_carry);
    }
    int64_t *d_ts, *d_pos, *d_rid;
    int32_t *d_s, *d_e, *d_dt;
    int16_t *d_b, *d_c;
    if ((rc = slot(c, S_TS, n, &d_ts)) || (rc = slot(c, S_POS, n, &d_pos)) || (rc = slot(c, S_START, n, &d_s)) ||
        (rc = slot(c, S_END, n, &d_e)) || (rc = slot(c, S_DT, n, &d_dt)) || (rc = slot(c, S_BOARD, n, &d_b)) ||
        (rc = slot(c, S_CHAN, n, &d_c)) || (rc = slot(c, S_RID, n, &d_rid)))
        return rc;
    hipLaunchKernelGGL(k_unpack_hit_rows, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, rows, (int64_t)60, d_ts, d_pos, d_s,
                       d_e, d_dt, d_b, d_c, d_rid);
    // 2. the sort and chain of the static entry over the whole table
    const HitCols h{d_ts, d_pos, d_s, d_e, d_dt, d_b, d_c, d_rid};
    int64_t n_cl = 0;
    int64_t* perm = nullptr;
    if ((rc = merge_cols(c, n, h, ms.gap_ns, ms.width_ns, &n_cl, &perm))) return rc;
    if (n_cl < 1 || n_cl > n) return fail(WFA_E_HIP, "merge stream: the chain reported %lld clusters of %lld hits", (long long)n_cl, (long long)n);
    // 3. the checks of the pushed rows, the closed clusters, the rows that stay; one read of the control block
    int64_t *closed, *closed_incl, *count, *comp_incl, *list, *keep, *keep_incl;
    MsCtl* d_ctl;
    if ((rc = slot(c, S_MS0, n_cl, &closed)) || (rc = slot(c, S_MS1, n_cl, &closed_incl)) || (rc = slot(c, S_MS2, n_cl, &count)) ||
        (rc = slot(c, S_MS3, n_cl, &comp_incl)) || (rc = slot(c, S_MS4, n_cl, &list)) || (rc = slot(c, S_K2, n, &keep)) ||
        (rc = slot(c, S_K3, n, &keep_incl)) || (rc = slot(c, S_MS5, 1, &d_ctl)))
        return rc;
    LaunchTimer t(c);
    MsCtl ctl{~0ull, ~0ull, 0, 0, 0, 0};
    WFA_HIP_CHECK(hipMemcpyAsync(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    if (n_rows > 0) {
        const unsigned cb = blocks_for(n_rows) < 1024u ? blocks_for(n_rows) : 1024u;
        hipLaunchKernelGGL(k_es_check<MsCtl>, dim3(cb), dim3(kTB), 0, c->stream, n_rows, d_dt + n_carry, d_s + n_carry,
                           d_e + n_carry, c->ht[S_ABS0].as<double>() + n_carry, d_ctl);
    }
    const int64_t* offset = c->ht[S_OUT0].as<int64_t>();
    const int64_t* cluster_incl = c->ht[S_ID].as<int64_t>();
    const double* s0 = c->ht[S_F0].as<double>();
    const double* s1 = c->ht[S_F1].as<double>();
    hipLaunchKernelGGL(k_ms_closed, dim3(blocks_for(n_cl)), dim3(kTB), 0, c->stream, n_cl, n, offset, s0, s1,
                       c->ht[S_SG].as<uint64_t>(), ms.gap_ns > 0 ? 1 : 0, ms.gap_ns * 1e3, horizon_ps, closed, count);
    if ((rc = plus_scan(c, closed, closed_incl, n_cl)) || (rc = plus_scan(c, count, comp_incl, n_cl))) return rc;
    hipLaunchKernelGGL(k_ms_keep, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, n_cl, perm, cluster_incl, closed, closed_incl,
                       comp_incl, s0, keep, d_ctl);
    WFA_HIP_CHECK(hipGetLastError());
    WFA_HIP_CHECK(hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (ctl.flags & kEsBadDt) return fail(WFA_E_INVALID, "hit dt must be positive for every row");
    if (ctl.flags & kEsBadEdge) return fail(WFA_E_INVALID, "a pushed row has a negative edge_start / edge_end");
    if (n_rows > 0 && ctl.min_key < host_ord_f64(ms.horizon))
        return fail(WFA_E_INVALID, "a pushed row starts below the previous push's horizon (%.17g ps)", ms.horizon);
    const int64_t n_closed = (int64_t)ctl.n_closed, n_comp = (int64_t)ctl.n_comp, n_keep = n - n_comp;
    if (n_closed < 0 || n_closed > n_cl || n_comp < n_closed || n_comp > n || (n_keep > 0) != (ctl.open_key != ~0ull))
        return fail(WFA_E_HIP, "merge stream: inconsistent counts");
    if (n_closed >= 0x80000000LL - io.out_used)
        return fail(WFA_E_INVALID, "carried merged rows (%lld) + closed clusters (%lld) reach the table limit of 2^31 rows",
                    (long long)io.out_used, (long long)n_closed);
    // 4. the merged rows and member indices of the closed clusters
    if (n_closed > 0) {
        float *height, *integral, *red_h, *red_int, *red_w;
        int32_t *red_s, *red_e;
        int64_t* anchor;
        const size_t entry = (size_t)io.out_words * 4;
        if ((rc = slot(c, S_HEIGHT, n, &height)) || (rc = slot(c, S_INTEGRAL, n, &integral)) || (rc = slot(c, S_OUT3, n_closed, &anchor)) ||
            (rc = slot(c, S_OUT4, n_closed, &red_h)) || (rc = slot(c, S_OUT5, n_closed, &red_int)) || (rc = slot(c, S_OUT6, n_closed, &red_s)) ||
            (rc = slot(c, S_OUT7, n_closed, &red_e)) || (rc = slot(c, S_MS6, n_closed, &red_w)) ||
            (rc = es_grow(c, *io.out, (size_t)io.out_used * entry, (size_t)(io.out_used + n_closed) * entry)) ||
            (rc = ms.out_index.ensure((size_t)n_comp * 8)))
            return rc;
        const uint32_t* words = reinterpret_cast<const uint32_t*>(rows);
        uint32_t* out = io.out->as<uint32_t>() + (size_t)io.out_used * io.out_words;
        hipLaunchKernelGGL(k_ms_cols, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, words, height, integral);
        hipLaunchKernelGGL(k_ms_list, dim3(blocks_for(n_cl)), dim3(kTB), 0, c->stream, n_cl, closed, closed_incl, list);
        hipLaunchKernelGGL(k_merge_emit, dim3(blocks_for(n_closed)), dim3(kTB), 0, c->stream, n_closed, offset, perm, h, height,
                           integral, anchor, red_h, red_int, red_s, red_e, red_w, list);
        hipLaunchKernelGGL(k_ms_rows, dim3(blocks_for(n_closed * 18)), dim3(kTB), 0, c->stream, n_closed, list, offset, comp_incl,
                           ms.next_component, anchor, red_h, red_int, red_s, red_e, red_w, words, out, io.out_words);
        if (io.out_words == 22)
            hipLaunchKernelGGL(k_mes_fix, dim3(blocks_for(n_closed)), dim3(kTB), 0, c->stream, n_closed, list, offset, s0, s1, red_s,
                               red_e, reinterpret_cast<double*>(out));
        hipLaunchKernelGGL(k_ms_members, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, perm, cluster_incl, closed, offset,
                           comp_incl, index, ms.out_index.as<int64_t>());
    }
    // 5. the hits of the open clusters and their indices, in row order, into the other buffers (all open: the table is
    //    the carry)
    if (n_keep > 0 && n_closed > 0 &&
        ((rc = plus_scan(c, keep, keep_incl, n)) || (rc = ms.carry.compact(c, n, keep, keep_incl, n_keep)) ||
         (rc = ms.index.compact(c, n, keep, keep_incl, n_keep))))
        return rc;
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("merge stream: closed clusters, rows, carry"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    r->n_closed = n_closed;
    r->n_comp = n_comp;
    r->n_keep = n_keep;
    r->open_start = n_keep > 0 ? host_unord_f64(ctl.open_key) : HUGE_VAL;
    r->flip = n_keep > 0 && n_closed > 0;
    return WFA_OK;
}

void merge_commit(wfa_ctx::MergeStream& ms, const MergeStepOut& r, int64_t n_rows, double horizon_ps) {
    ms.carry.commit(r.n_keep, r.flip);
    ms.index.commit(r.n_keep, r.flip);
    ms.next_hit += n_rows;
    ms.next_component += r.n_comp;
    ms.horizon = horizon_ps;
    ms.out_merged = r.n_closed;
    ms.out_components = r.n_comp;
}

// what the group step and the df step decide
struct GroupStepOut {
    int64_t n_out = 0, n_closed = 0, n_keep = 0;
    bool flip = false;  // the carry went to the other buffer
};

// The group step over the table of es.carry: the carried entries, then n_new new ones, already in place (n = both > 0;
// the caller has checked the horizon).  An entry is S dwords; its first W are the row that goes out behind
// the three event fields, and where S > W it ends with the row's abs_start_fix / abs_end_fix (S = 22, W = 18: a merged
// row, whose edges may be -1, -1; S = W = 15: a threshold hit, whose edges may not).
template <int W, int S>
int group_step(wfa_ctx* c, wfa_ctx::EventStream& es, int64_t n_new, double horizon_ps, GroupStepOut* r) {
    int rc;
    *r = GroupStepOut{};
    if (es.carry.row != S * 4) return fail(WFA_E_INVALID, "group step: %d-dword entries on a carry of %d-byte rows", S, es.carry.row);
    const int64_t n_carry = es.carry.n, n = n_carry + n_new;
    c->ht_n = -1;  // the scratch slots a static count pass left for its fill are overwritten
    uint8_t* rows = es.carry.table().as<uint8_t>();
    int64_t *d_ts, *d_pos, *d_rid;
    int32_t *d_s, *d_e, *d_dt;
    int16_t *d_b, *d_c;
    double *ev_hi, *fix0 = nullptr, *fix1 = nullptr;
    EsCtl* d_ctl;
    if ((rc = slot(c, S_TS, n, &d_ts)) || (rc = slot(c, S_POS, n, &d_pos)) || (rc = slot(c, S_START, n, &d_s)) ||
        (rc = slot(c, S_END, n, &d_e)) || (rc = slot(c, S_DT, n, &d_dt)) || (rc = slot(c, S_BOARD, n, &d_b)) ||
        (rc = slot(c, S_CHAN, n, &d_c)) || (rc = slot(c, S_RID, n, &d_rid)) || (rc = slot(c, S_EVHI, n, &ev_hi)) ||
        (rc = slot(c, S_ES, 1, &d_ctl)))
        return rc;
    hipLaunchKernelGGL(k_unpack_hit_rows, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, rows, (int64_t)(S * 4), d_ts, d_pos,
                       d_s, d_e, d_dt, d_b, d_c, d_rid);
    if (S > W) {
        if ((rc = slot(c, S_OUT6, n, &fix0)) || (rc = slot(c, S_OUT7, n, &fix1))) return rc;
        hipLaunchKernelGGL(k_mes_fixcols, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, reinterpret_cast<const double*>(rows),
                           fix0, fix1);
    }
    // the grouping pass of the static entry over the whole table
    const HitCols h{d_ts, d_pos, d_s, d_e, d_dt, d_b, d_c, d_rid};
    int64_t n_ev = 0;
    int64_t* perm = nullptr;
    if ((rc = group_cols(c, n, h, fix0, fix1, es.window_ns, &n_ev, &perm, ev_hi))) return rc;
    if (n_ev < 1 || n_ev > n) return fail(WFA_E_HIP, "event stream: the grouping pass reported %lld events of %lld hits", (long long)n_ev, (long long)n);
    // the checks of the new rows and the closed prefix; one read of the control block
    LaunchTimer t(c);
    EsCtl ctl{~0ull, (unsigned long long)n_ev, 0, 0, 0};
    WFA_HIP_CHECK(hipMemcpyAsync(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    const double* abs0 = c->ht[S_ABS0].as<double>();
    if (n_new > 0) {
        const unsigned cb = blocks_for(n_new) < 1024u ? blocks_for(n_new) : 1024u;
        hipLaunchKernelGGL(k_es_check<EsCtl>, dim3(cb), dim3(kTB), 0, c->stream, n_new, d_dt + n_carry, d_s + n_carry,
                           d_e + n_carry, abs0 + n_carry, d_ctl);
    }
    const int64_t* ev_start = c->ht[S_OUT0].as<int64_t>();
    hipLaunchKernelGGL(k_es_closed, dim3(blocks_for(n_ev)), dim3(kTB), 0, c->stream, n_ev, ev_hi, es.window_ns * 1e3, horizon_ps,
                       d_ctl);
    hipLaunchKernelGGL(k_es_count, dim3(1), dim3(64), 0, c->stream, ev_start, d_ctl);
    WFA_HIP_CHECK(hipGetLastError());
    WFA_HIP_CHECK(hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (ctl.flags & kEsBadDt) return fail(WFA_E_INVALID, "hit dt must be positive for every row");
    if (S == W && (ctl.flags & kEsBadEdge))  // (merged rows come from the merge step, which has checked the hits' edges)
        return fail(WFA_E_INVALID, "a pushed row has a negative edge_start / edge_end (merged hits that span records are "
                                   "outside the event stream)");
    if (n_new > 0 && ctl.min_key < host_ord_f64(es.horizon))
        return fail(WFA_E_INVALID, "a pushed row starts below the previous push's horizon (%.17g ps)", es.horizon);
    const int64_t n_closed = (int64_t)ctl.n_closed, n_out = (int64_t)ctl.n_out, n_keep = n - n_out;
    if (n_closed < 0 || n_closed > n_ev || n_out < 0 || n_out > n) return fail(WFA_E_HIP, "event stream: inconsistent counts");
    // the rows of the closed events
    const uint64_t* k_ev = c->ht[S_K1].as<uint64_t>();
    if (n_out > 0) {
        if ((rc = es.out.ensure((size_t)n_out * (6 + W) * 4))) return rc;
        hipLaunchKernelGGL((k_es_rows<W, S>), dim3(blocks_for(n_out * (6 + W))), dim3(kTB), 0, c->stream, n_out, perm, k_ev,
                           c->ht[S_OUT1].as<int64_t>(), c->ht[S_OUT2].as<int64_t>(), es.next_event,
                           reinterpret_cast<const uint32_t*>(rows), es.out.as<uint32_t>());
    }
    // the entries of the open events, in row order, into the other carry buffer (all open: the table is the carry)
    if (n_keep > 0 && n_out > 0) {
        int64_t* flag = c->ht[S_FLAG].as<int64_t>();
        int64_t* incl = c->ht[S_ID].as<int64_t>();
        hipLaunchKernelGGL(k_es_keep, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, k_ev, n_closed, flag);
        size_t tb = c->ht[S_CUB].cap;  // (sized by group_cols for this very scan)
        WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, flag, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
        if ((rc = es.carry.compact(c, n, flag, incl, n_keep))) return rc;
    }
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("event stream: closed prefix, rows, carry"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    r->n_out = n_out;
    r->n_closed = n_closed;
    r->n_keep = n_keep;
    r->flip = n_keep > 0 && n_out > 0;
    return WFA_OK;
}

// (Stream: the event stream's state or the df_events stream's, H its horizon type)
template <typename Stream, typename H>
void group_commit(Stream& st, const GroupStepOut& r, H horizon) {
    st.carry.commit(r.n_keep, r.flip);
    st.next_event += r.n_closed;
    st.horizon = horizon;
    st.out_rows = r.n_out;
}

// rows of a finished push to the host (large ones through the pinned staging ring); the caller synchronises
int stream_d2h(wfa_ctx* c, void* dst, const void* src, size_t bytes) {
    if (bytes >= (4u << 20)) return d2h_staged(c, dst, src, bytes, nullptr, nullptr);
    WFA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return WFA_OK;
}

// ---- df_events stream (wfa_df_event_stream_*) -------------------------------------------------------------------------
// The fixed-window grouping chunk by chunk.  A push chains carry ++ new rows like wfa_group_multi_channel_count (stable
// sort by timestamp, next search, pointer jumping) and closes the events whose anchor a has (double)H > (double)a + window,
// strictly, or all of them when the push is final.  Anchors ascend and the float64 sum is monotone, so the closed events
// are a prefix of the chain, and since an event is a run of the timestamp order, their rows are the sorted positions
// [0, n_out) with n_out = the position of the first open anchor: one number says which events close, which rows go out
// and which stay.  Only that prefix is sorted again by (event, channel).
constexpr int kDfsBadReserved = 1;
struct DfsCtl {
    unsigned long long min_key;     // ord_i64 of the smallest timestamp among the pushed rows
    unsigned long long first_open;  // sorted position of the first open event's anchor; n: every event closes
    long long n_closed;             // events of the closed prefix
    int flags, pad;
};

// 40-byte rows as 5 qwords: timestamp @0, record_id @1, area | height @2, amp | max_abs_diff @3, board | channel | reserved @4.
// The timestamp and channel columns of the whole table for the chain; of the pushed rows [n_carry, n) the smallest
// timestamp and the reserved check
__global__ __launch_bounds__(kTB) void k_dfs_cols(int64_t n, int64_t n_carry, const int64_t* __restrict__ rows,
                                                  int64_t* __restrict__ ts, int64_t* __restrict__ ch,
                                                  DfsCtl* __restrict__ ctl) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    unsigned long long lo = ~0ull;
    int bad = 0;
    if (i < n) {
        const int64_t t = rows[i * 5];
        const uint64_t tail = (uint64_t)rows[i * 5 + 4];
        ts[i] = t;
        ch[i] = (int64_t)(int16_t)(uint16_t)(tail >> 16);
        if (i >= n_carry) {
            lo = ord_i64(t);
            if (tail >> 32) bad = kDfsBadReserved;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, d);
        lo = ol < lo ? ol : lo;
        bad |= __shfl_xor(bad, d);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo != ~0ull) atomicMin(&ctl->min_key, lo);
        if (bad) atomicOr(&ctl->flags, bad);
    }
}

// the close rule over the anchors (the marked sorted positions): open <=> not final and not (double)H > anchor + window
__global__ __launch_bounds__(kTB) void k_dfs_closed(int64_t n, const int64_t* __restrict__ mark,
                                                    const double* __restrict__ ts_f, double window_ps, double horizon,
                                                    int final, DfsCtl* __restrict__ ctl) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    unsigned long long lo = ~0ull;
    if (j < n && !final && mark[j] && !(horizon > ts_f[j] + window_ps)) lo = (unsigned long long)j;
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long ol = __shfl_xor(lo, d);
        lo = ol < lo ? ol : lo;
    }
    if ((threadIdx.x & 63) == 0 && lo != ~0ull) atomicMin(&ctl->first_open, lo);
}
// events before the first open anchor (incl = the inclusive scan of the marks)
__global__ void k_dfs_count(int64_t n, const int64_t* __restrict__ incl, DfsCtl* __restrict__ ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long fo = ctl->first_open;
    ctl->n_closed = fo >= (unsigned long long)n ? incl[n - 1] : incl[fo] - 1;
}

// one key for the (event, channel) order of the closed prefix [0, n_out) of the timestamp order: the event index above
// the 16 bits of the int16 channel
__global__ void k_dfs_keys(int64_t n_out, const int64_t* __restrict__ perm, const int64_t* __restrict__ incl,
                           const int64_t* __restrict__ ch, uint64_t* __restrict__ key) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j < n_out) key[j] = ((uint64_t)(incl[j] - 1) << 16) | ((uint64_t)(ch[perm[j]] + 32768) & 0xffffu);
}

// 64-byte rows as 16 dwords, lanes over dwords: event_id, t_min, t_max (6 dwords), the input row's first 8 dwords
// (timestamp .. max_abs_diff), n_hits, board | channel.  Output row p is sorted position order[p] = table row
// perm[order[p]]; event e holds the output rows [bounds[e], bounds[e + 1]) and t_min / t_max are the timestamps of its
// first and last output row (after the channel sort: not the extremes)
__global__ __launch_bounds__(kTB) void k_dfs_rows(int64_t n_out, const int64_t* __restrict__ order,
                                                  const int64_t* __restrict__ perm, const int64_t* __restrict__ incl,
                                                  const int64_t* __restrict__ bounds, int64_t first_event,
                                                  const uint32_t* __restrict__ rows, uint32_t* __restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (d >= n_out * 16) return;
    const int64_t p = d >> 4;
    const int w = (int)(d & 15);
    const int64_t q = order[p];
    const int64_t i = perm[q];
    if (w >= 6 && w < 14) { out[d] = rows[i * 10 + (w - 6)]; return; }
    if (w == 15) { out[d] = rows[i * 10 + 8]; return; }
    const int64_t ev = incl[q] - 1;
    const int64_t a = bounds[ev], b = bounds[ev + 1];
    if (w == 14) { out[d] = (uint32_t)(b - a); return; }
    const int64_t edge = perm[order[w < 4 ? a : b - 1]];
    const uint32_t* src = rows + edge * 10;
    const int64_t v = w < 2 ? first_event + ev : (int64_t)((uint64_t)src[0] | ((uint64_t)src[1] << 32));
    out[d] = (w & 1) ? (uint32_t)((uint64_t)v >> 32) : (uint32_t)(uint64_t)v;
}

// keep flag per table row: 1 where its sorted position lies behind the closed prefix
__global__ void k_dfs_keep(int64_t n, int64_t n_out, const int64_t* __restrict__ perm, int64_t* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (j < n) flag[perm[j]] = j >= n_out ? 1 : 0;
}

// One push over the table of ds.carry: the carried rows, then the pushed ones.  Reads the stream's counters and changes
// none of them; the caller commits.
int dfs_step(wfa_ctx* c, wfa_ctx::DfEventStream& ds, const void* rows_in, int64_t n_rows, int64_t horizon_ts, int final,
             GroupStepOut* r) {
    int rc;
    *r = GroupStepOut{};
    const int64_t n = ds.carry.n + n_rows;
    if (n == 0) return WFA_OK;  // nothing carried, nothing pushed: no launch
    c->ht_n = -1;  // the scratch slots a static count pass left for its fill are overwritten
    if ((rc = ds.carry.reserve(c, n_rows)) || (rc = ds.carry.upload(c, rows_in, n_rows))) return rc;
    const DevBuf& table = ds.carry.table();
    int levels = 1;
    while ((1ll << levels) < n) ++levels;  // next^(2^levels) of any row is n
    int64_t *ts, *ch, *mark, *incl;
    uint64_t *k_ts, *k_ch;
    double* ts_f;
    int32_t* jump;  // two levels, J_k and J_(k+1), used in turn
    DfsCtl* d_ctl;
    if ((rc = slot(c, S_TS, n, &ts)) || (rc = slot(c, S_POS, n, &ch)) || (rc = slot(c, S_K0, n, &k_ts)) ||
        (rc = slot(c, S_K1, n, &k_ch)) || (rc = slot(c, S_ABS0, n, &ts_f)) || (rc = slot(c, S_FLAG, n, &mark)) ||
        (rc = slot(c, S_ID, n, &incl)) || (rc = slot(c, S_OUT3, 2 * (n + 1), &jump)) || (rc = slot(c, S_ES, 1, &d_ctl)))
        return rc;
    LaunchTimer t(c);
    DfsCtl ctl{~0ull, (unsigned long long)n, 0, 0, 0};
    WFA_HIP_CHECK(hipMemcpyAsync(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dfs_cols, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, ds.carry.n, table.as<int64_t>(), ts, ch, d_ctl);
    // the chain of the static pass over the whole table (k_mc_keys as the static pass launches it: its channel key is not
    // read here, the closed prefix gets a key of its own below)
    hipLaunchKernelGGL(k_mc_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, ts, ch, k_ts, k_ch);
    int64_t* perm = nullptr;
    {
        const uint64_t* keys[1] = {k_ts};  // stable: the carry stands in front of the pushed rows, as in the whole table
        if ((rc = lexsort(c, n, keys, 1, &perm))) return rc;  // (its wait covers the upload of `ctl`)
    }
    hipLaunchKernelGGL(k_mc_sorted_ts, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, ts, perm, ts_f);
    hipLaunchKernelGGL(k_mc_next, dim3(blocks_for(n + 1)), dim3(kTB), 0, c->stream, n, ts_f, ds.window_ps, jump);
    WFA_HIP_CHECK(hipMemsetAsync(mark, 0, (size_t)n * sizeof(int64_t), c->stream));
    static const int64_t one = 1;
    WFA_HIP_CHECK(hipMemcpyAsync(mark, &one, sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < levels; ++k)
        hipLaunchKernelGGL(k_mc_mark_jump, dim3(blocks_for(n + 1)), dim3(kTB), 0, c->stream, n, jump + (int64_t)(k & 1) * (n + 1),
                           jump + (int64_t)((k + 1) & 1) * (n + 1), mark);
    if ((rc = plus_scan(c, mark, incl, n))) return rc;
    // the close rule, the prefix count, the checks of the pushed rows; one read of the control block
    hipLaunchKernelGGL(k_dfs_closed, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, mark, ts_f, ds.window_ps, (double)horizon_ts,
                       final ? 1 : 0, d_ctl);
    hipLaunchKernelGGL(k_dfs_count, dim3(1), dim3(64), 0, c->stream, n, incl, d_ctl);
    WFA_HIP_CHECK(hipGetLastError());
    WFA_HIP_CHECK(hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (ctl.flags & kDfsBadReserved) return fail(WFA_E_INVALID, "a pushed row has reserved != 0");
    if (n_rows > 0 && ctl.min_key < ((uint64_t)ds.horizon ^ 0x8000000000000000ull))
        return fail(WFA_E_INVALID, "a pushed row's timestamp lies below the previous push's horizon (%lld ps)", (long long)ds.horizon);
    const int64_t n_out = ctl.first_open < (unsigned long long)n ? (int64_t)ctl.first_open : n;
    const int64_t n_closed = (int64_t)ctl.n_closed, n_keep = n - n_out;
    if (n_closed < 0 || n_closed > n_out || (n_closed == 0) != (n_out == 0))
        return fail(WFA_E_HIP, "df_events stream: inconsistent counts");
    if (n_out > 0) {
        // the (event, channel) order of the closed prefix (the second sort takes lexsort's buffers: the timestamp order
        // moves out of them first), the events' bounds in it, the rows
        int64_t *perm_ts, *bounds, *order = nullptr;
        uint64_t* key;
        if ((rc = slot(c, S_OUT1, n, &perm_ts)) || (rc = slot(c, S_K2, n_out, &key)) || (rc = slot(c, S_OUT0, n_closed + 1, &bounds)) ||
            (rc = ds.out.ensure((size_t)n_out * 64)))
            return rc;
        WFA_HIP_CHECK(hipMemcpyAsync(perm_ts, perm, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_dfs_keys, dim3(blocks_for(n_out)), dim3(kTB), 0, c->stream, n_out, perm_ts, incl, ch, key);
        {
            const uint64_t* keys[1] = {key};
            if ((rc = lexsort(c, n_out, keys, 1, &order))) return rc;
        }
        hipLaunchKernelGGL(k_mc_bounds, dim3(blocks_for(n_out)), dim3(kTB), 0, c->stream, n_out, mark, incl, n_closed, bounds);
        hipLaunchKernelGGL(k_dfs_rows, dim3(blocks_for(n_out * 16)), dim3(kTB), 0, c->stream, n_out, order, perm_ts, incl, bounds,
                           ds.next_event, table.as<uint32_t>(), ds.out.as<uint32_t>());
        // the rows of the open events, in row order, into the other carry buffer (all open: the table is the carry)
        if (n_keep > 0) {
            int64_t *keep, *keep_incl;
            if ((rc = slot(c, S_K3, n, &keep)) || (rc = slot(c, S_K4, n, &keep_incl))) return rc;
            hipLaunchKernelGGL(k_dfs_keep, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, n_out, perm_ts, keep);
            if ((rc = plus_scan(c, keep, keep_incl, n)) || (rc = ds.carry.compact(c, n, keep, keep_incl, n_keep))) return rc;
        }
    }
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("df_events stream: chain, closed prefix, rows, carry"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    r->n_out = n_out;
    r->n_closed = n_closed;
    r->n_keep = n_keep;
    r->flip = n_keep > 0 && n_out > 0;
    return WFA_OK;
}

// ---- records stream (wfa_records_stream_*) ----------------------------------------------------------------------------
// records and wave_pool from V1725 blocks, block by block.  The table of a push is the carried entries, then the pushed
// waves; it is ordered by (timestamp, board, channel, seq) -- seq is a key: a carried wave of a later file and a pushed one
// of an earlier file may tie on the first three -- and the waves with timestamp < horizon (all, when final) are a prefix
// of that order.  The inclusive scan of the lengths in that order places every wave's samples: the prefix in the output
// pool, the rest in the new sample carry.  Entry = 5 qwords: timestamp, seq, sample offset (carried: into the sample carry;
// pushed: into the block; in samples, even), n_samples | board << 32 | channel << 48, baseline | trunc << 16.
struct RsCtl {
    unsigned long long n_out;   // waves of the released prefix
    long long out_samples;      // their samples
    long long total_samples;    // samples of the whole table
};

__global__ void k_rs_keys(int64_t n, const int64_t* __restrict__ rows, uint64_t* __restrict__ k_ts, uint64_t* __restrict__ k_bc,
                          uint64_t* __restrict__ k_seq) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const uint64_t q3 = (uint64_t)rows[i * 5 + 3];
    k_ts[i] = ord_i64(rows[i * 5]);
    k_seq[i] = ord_i64(rows[i * 5 + 1]);
    k_bc[i] = ((uint64_t)((uint16_t)(q3 >> 32) ^ 0x8000u) << 16) | (uint64_t)((uint16_t)(q3 >> 48) ^ 0x8000u);
}

// lengths in sorted order, and the size of the released prefix
__global__ __launch_bounds__(kTB) void k_rs_lengths(int64_t n, const int64_t* __restrict__ perm, const int64_t* __restrict__ rows,
                                                    int64_t horizon, int final, int64_t* __restrict__ len, RsCtl* __restrict__ ctl) {
    const int64_t j = (int64_t)blockIdx.x * kTB + threadIdx.x;
    bool out = false;
    if (j < n) {
        const int64_t t = perm[j];
        len[j] = (int64_t)(uint32_t)(uint64_t)rows[t * 5 + 3];
        out = final || rows[t * 5] < horizon;
    }
    const unsigned long long m = __ballot(out);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl->n_out, (unsigned long long)__popcll(m));
}
__global__ void k_rs_totals(int64_t n, const int64_t* __restrict__ incl, RsCtl* __restrict__ ctl) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long k = ctl->n_out;
    ctl->out_samples = k > 0 ? incl[k - 1] : 0;
    ctl->total_samples = incl[n - 1];
}

// The sample pass.  Output-stationary: a lane owns 16 bytes (8 samples) of a destination -- the output pool (region 0: the
// released prefix) or the new sample carry (region 1: the rest) -- and stores them with one aligned dwordx4 store; the
// buffers are padded to whole chunks and the bytes behind a region's last sample are written as 0.  Every source and
// destination offset and every length is an even number of samples, so a destination dword is exactly one source dword:
// the source is read as dwords at 4-byte alignment (four adjacent ones when the chunk lies inside one wave, which the
// hardware takes as one 16-byte load), never as halfwords.  A wave64 owns kRsTiles consecutive tiles of 64 chunks of one
// region (region 1 starts on a wave64 boundary of the index space).  Per tile it finds the waves of the tile's first and last
// dword, wave-uniformly, in the scanned lengths -- one binary search for its first tile, then galloping on from where the
// tile before ended (one probe when the next tile starts in the same or the next wave: a search per 1 KiB kept the pass at
// a third of the copy rate) -- and each lane searches between those two: no step at all when the 512 samples lie in one
// wave, and short waves cost a few steps instead of idle lanes.  Zero-sample waves own no dword and are never found.
struct RsMoveArgs {
    const int64_t* incl;        // inclusive scan of the lengths in sorted order
    const int64_t* perm;        // sorted position -> table row
    const int64_t* rows;        // the table
    int64_t n, n_out, n_carry;  // table rows, released prefix, rows [0, n_carry) of the table read the sample carry
    int64_t out_samples, total_samples;
    int64_t out_waves;          // wave64s of region 0
    int64_t n_waves;            // wave64s of both regions
    const uint32_t* src_carry;
    const uint32_t* src_block;
    uint4* dst_out;
    uint4* dst_keep;
};
constexpr int kRsBlock = 256;
constexpr int kRsTiles = 8;  // 1-KiB tiles a wave64 moves one after another: one search, then a short walk per tile
constexpr int kWave = 64;
__device__ __forceinline__ int lane_id() { return threadIdx.x & (kWave - 1); }
__device__ __forceinline__ int wave_in_block() { return threadIdx.x >> 6; }
__device__ __forceinline__ int64_t uniform_i64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// first j in [lo, hi) with incl[j] > p; hi when there is none
__device__ __forceinline__ int64_t rs_find(const int64_t* __restrict__ incl, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (incl[mid] > p) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// the same, from a start that is usually already the answer: probe lo, lo + 1, lo + 3, lo + 7, ... then bisect the last gap
__device__ __forceinline__ int64_t rs_gallop(const int64_t* __restrict__ incl, int64_t lo, int64_t hi, int64_t p) {
    int64_t at = lo, step = 1;
    while (at < hi && incl[at] <= p) {
        lo = at + 1;
        at += step;
        step <<= 1;
    }
    return rs_find(incl, lo, at < hi ? at : hi, p);
}

struct RsSrcA4 {  // four adjacent dwords at 4-byte alignment
    uint32_t x, y, z, w;
} __attribute__((packed, aligned(4)));

__global__ __launch_bounds__(kRsBlock) void k_rs_move(RsMoveArgs a) {
    const int lane = lane_id();
    const int64_t w = uniform_i64((int64_t)blockIdx.x * (kRsBlock / kWave) + wave_in_block());
    if (w >= a.n_waves) return;
    const bool keep = w >= a.out_waves;
    const int64_t c0 = (keep ? w - a.out_waves : w) * (kWave * kRsTiles);  // first chunk of the wave64 in its region
    const int64_t base = keep ? a.out_samples : 0;                          // the region in the scan's sample axis: [base, lim)
    const int64_t lim = keep ? a.total_samples : a.out_samples;
    const int64_t jhi = keep ? a.n : a.n_out;
    int64_t jcur = keep ? a.n_out : 0;   // no wave in front of it holds a sample of this tile or a later one
    uint4* __restrict__ dst = keep ? a.dst_keep : a.dst_out;
#pragma unroll 1
    for (int tile = 0; tile < kRsTiles; ++tile) {
        const int64_t p0 = base + (c0 + (int64_t)tile * kWave) * 8;
        if (p0 >= lim) break;
        const int64_t p_last = (p0 + kWave * 8 < lim ? p0 + kWave * 8 : lim) - 2;
        const int64_t j0 = uniform_i64(tile == 0 ? rs_find(a.incl, jcur, jhi, p0) : rs_gallop(a.incl, jcur, jhi, p0));
        const int64_t j1 = uniform_i64(rs_gallop(a.incl, j0, jhi, p_last));  // (< jhi: p_last lies in a wave of the region)
        jcur = j1;
        const int64_t p = p0 + lane * 8;
        if (p >= lim) continue;
        int64_t j = j0 == j1 ? j0 : rs_find(a.incl, j0, j1, p);
        uint32_t o[4];
        int64_t end = a.incl[j];
        int64_t t = a.perm[j];
        int64_t off = a.rows[t * 5 + 2];
        int64_t first = end - (int64_t)(uint32_t)(uint64_t)a.rows[t * 5 + 3];  // the wave's first sample on the scan's axis
        const uint32_t* __restrict__ src = t < a.n_carry ? a.src_carry : a.src_block;
        if (p + 8 <= end) {
            const RsSrcA4 v = *reinterpret_cast<const RsSrcA4*>(src + ((off + (p - first)) >> 1));
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int64_t pd = p + 2 * d;
                uint32_t v = 0;
                if (pd < lim) {
                    if (pd >= end) {
                        do { ++j; end = a.incl[j]; } while (pd >= end);   // (ends at j1 at the latest)
                        t = a.perm[j];
                        off = a.rows[t * 5 + 2];
                        first = end - (int64_t)(uint32_t)(uint64_t)a.rows[t * 5 + 3];
                        src = t < a.n_carry ? a.src_carry : a.src_block;
                    }
                    v = src[(off + (pd - first)) >> 1];
                }
                o[d] = v;
            }
        }
        dst[(p - base) >> 3] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// the released prefix as packed 102-byte RECORDS_DTYPE rows, 51 halfwords each (fields behind trigger_type are only
// 2-byte aligned); lanes over halfwords: timestamp 0, pid 4, board 6, channel 7, baseline 8, baseline_upstream 12,
// polarity 16 (8 UCS-4), record_id 32, dt 36, trigger_type 38, flags 39, wave_offset 41, event_length 45, time 47
__global__ __launch_bounds__(kTB) void k_rs_rows(int64_t n_out, const int64_t* __restrict__ perm, const int64_t* __restrict__ incl,
                                                 const int64_t* __restrict__ rows, int64_t next_record, int64_t next_sample,
                                                 int32_t dt_ns, uint16_t* __restrict__ out) {
    const int64_t d = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (d >= n_out * 51) return;
    const int64_t j = d / 51;
    const int h = (int)(d - j * 51);
    const int64_t* __restrict__ e = rows + perm[j] * 5;
    const uint64_t q3 = (uint64_t)e[3];
    uint64_t v = 0;
    int k = 0;
    if (h < 4) { v = (uint64_t)e[0]; k = h; }
    else if (h < 6) { v = 0; }                                                       // pid
    else if (h == 6) { v = (q3 >> 32) & 0xffffu; }
    else if (h == 7) { v = q3 >> 48; }
    else if (h < 12) { v = (uint64_t)__double_as_longlong((double)(uint32_t)((uint64_t)e[4] & 0xffffu)); k = h - 8; }
    else if (h < 16) { v = 0x7ff8000000000000ull; k = h - 12; }                      // numpy's nan
    else if (h < 32) {
        const int cp = (h - 16) >> 1;
        v = ((h & 1) == 0 && cp < 7) ? (uint64_t)(uint8_t)"unknown"[cp] : 0;
    }
    else if (h < 36) { v = (uint64_t)(next_record + j); k = h - 32; }
    else if (h < 38) { v = (uint32_t)dt_ns; k = h - 36; }
    else if (h == 38) { v = 0; }                                                     // trigger_type
    else if (h < 41) { v = ((uint64_t)e[4] >> 16) & 0xffu; k = h - 39; }            // flags = trunc
    else if (h < 45) { v = (uint64_t)(next_sample + incl[j] - (int64_t)(uint32_t)q3); k = h - 41; }
    else if (h < 47) { v = (uint32_t)q3; k = h - 45; }
    else {
        const int64_t ts = e[0];
        int64_t q = ts / 1000;
        if (ts - q * 1000 < 0) --q;   // floor, as numpy's //
        v = (uint64_t)q;
        k = h - 47;
    }
    out[d] = (uint16_t)(v >> (16 * k));
}

// the entries behind the released prefix, in sorted order, into the other carry buffer; their samples now lie in the new
// sample carry at the scan's offsets
__global__ void k_rs_keep(int64_t n_keep, int64_t n_out, int64_t out_samples, const int64_t* __restrict__ perm,
                          const int64_t* __restrict__ incl, const int64_t* __restrict__ rows, int64_t* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * kTB + threadIdx.x;
    if (i >= n_keep) return;
    const int64_t j = n_out + i;
    const int64_t* __restrict__ e = rows + perm[j] * 5;
    dst[i * 5] = e[0];
    dst[i * 5 + 1] = e[1];
    dst[i * 5 + 2] = incl[j] - (int64_t)(uint32_t)(uint64_t)e[3] - out_samples;
    dst[i * 5 + 3] = e[3];
    dst[i * 5 + 4] = e[4];
}

struct RecordsStepOut {
    int64_t n_out = 0, out_samples = 0, n_keep = 0, keep_samples = 0;
    bool flip = false;
};

// One push over the table of rs.carry (the pushed waves already packed in rs.pack and checked).  Reads the stream's
// counters and changes none of them; the caller commits.
int records_step(wfa_ctx* c, wfa_ctx::RecordsStream& rs, const uint8_t* block, int64_t n_bytes, int64_t n_new, int64_t horizon_ps,
                 int final, RecordsStepOut* r) {
    int rc;
    *r = RecordsStepOut{};
    const int64_t n_carry = rs.carry.n, n = n_carry + n_new;
    if (n == 0) return WFA_OK;  // nothing carried, nothing pushed: no launch
    c->ht_n = -1;  // the scratch slots a static count pass left for its fill are overwritten
    if ((rc = rs.carry.reserve(c, n_new)) || (rc = rs.carry.upload(c, rs.pack.data(), n_new))) return rc;
    if (n_new > 0 && n_bytes > 0) {
        const size_t padded = ((size_t)n_bytes + 3) & ~(size_t)3;
        if ((rc = rs.block.ensure(padded)) || (rc = h2d_copy(c, rs.block.ptr, block, (size_t)n_bytes))) return rc;
    }
    const int64_t* table = rs.carry.table().as<int64_t>();
    uint64_t *k_ts, *k_bc, *k_seq;
    int64_t *len, *incl;
    RsCtl* d_ctl;
    if ((rc = slot(c, S_K0, n, &k_ts)) || (rc = slot(c, S_K1, n, &k_bc)) || (rc = slot(c, S_K2, n, &k_seq)) ||
        (rc = slot(c, S_FLAG, n, &len)) || (rc = slot(c, S_ID, n, &incl)) || (rc = slot(c, S_ES, 1, &d_ctl)))
        return rc;
    LaunchTimer t(c);
    RsCtl ctl{0ull, 0, 0};
    WFA_HIP_CHECK(hipMemcpyAsync(d_ctl, &ctl, sizeof(ctl), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_rs_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, table, k_ts, k_bc, k_seq);
    int64_t* perm = nullptr;
    {
        const uint64_t* keys[3] = {k_ts, k_bc, k_seq};
        if ((rc = lexsort(c, n, keys, 3, &perm))) return rc;  // (its wait covers the upload of `ctl`)
    }
    hipLaunchKernelGGL(k_rs_lengths, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, perm, table, horizon_ps, final ? 1 : 0, len,
                       d_ctl);
    if ((rc = plus_scan(c, len, incl, n))) return rc;
    hipLaunchKernelGGL(k_rs_totals, dim3(1), dim3(64), 0, c->stream, n, incl, d_ctl);
    WFA_HIP_CHECK(hipGetLastError());
    WFA_HIP_CHECK(hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int64_t n_out = (int64_t)ctl.n_out, n_keep = n - n_out;
    const int64_t out_samples = ctl.out_samples, keep_samples = ctl.total_samples - ctl.out_samples;
    if (n_out < 0 || n_out > n || out_samples < 0 || keep_samples < 0 || (out_samples & 1) || (keep_samples & 1))
        return fail(WFA_E_HIP, "records stream: inconsistent counts");
    if ((rc = t.end("records stream: order, released prefix, offsets"))) return rc;
    // whole 16-byte chunks: the sample pass stores nothing narrower
    const int64_t out_chunks = (out_samples + 7) >> 3, keep_chunks = (keep_samples + 7) >> 3;
    DevBuf& new_samples = rs.samples[rs.cur_s ^ 1];
    DevBuf& new_carry = rs.carry.buf[rs.carry.cur ^ 1];
    if ((rc = rs.out_pool.ensure((size_t)(out_chunks > 0 ? out_chunks : 1) * 16)) ||
        (rc = rs.out_rows.ensure((size_t)(n_out > 0 ? n_out : 1) * 102 + 2)))
        return rc;
    if (n_keep > 0 && ((rc = new_samples.ensure((size_t)(keep_chunks > 0 ? keep_chunks : 1) * 16)) ||
                       (rc = new_carry.ensure((size_t)n_keep * 40))))
        return rc;
    if (out_chunks + keep_chunks > 0) {
        RsMoveArgs a{};
        a.incl = incl; a.perm = perm; a.rows = table;
        a.n = n; a.n_out = n_out; a.n_carry = n_carry;
        a.out_samples = out_samples; a.total_samples = ctl.total_samples;
        a.out_waves = (out_chunks + kWave * kRsTiles - 1) / (kWave * kRsTiles);
        a.n_waves = a.out_waves + (keep_chunks + kWave * kRsTiles - 1) / (kWave * kRsTiles);
        a.src_carry = rs.samples[rs.cur_s].as<uint32_t>();
        a.src_block = rs.block.as<uint32_t>();
        a.dst_out = rs.out_pool.as<uint4>();
        a.dst_keep = new_samples.as<uint4>();
        const int64_t grid = (a.n_waves + (kRsBlock / kWave) - 1) / (kRsBlock / kWave);
        if (grid > 0x7fffffff) return fail(WFA_E_LIMIT, "records stream: a push moves too many samples for one launch");
        LaunchTimer tm(c, true);
        hipLaunchKernelGGL(k_rs_move, dim3((unsigned)grid), dim3(kRsBlock), 0, c->stream, a);
        WFA_HIP_CHECK(hipGetLastError());
        if ((rc = tm.end("k_rs_move"))) return rc;
    }
    LaunchTimer t2(c);
    if (n_out > 0)
        hipLaunchKernelGGL(k_rs_rows, dim3(blocks_for(n_out * 51)), dim3(kTB), 0, c->stream, n_out, perm, incl, table, rs.next_record,
                           rs.next_sample, rs.dt_ns, rs.out_rows.as<uint16_t>());
    if (n_keep > 0)
        hipLaunchKernelGGL(k_rs_keep, dim3(blocks_for(n_keep)), dim3(kTB), 0, c->stream, n_keep, n_out, out_samples, perm, incl, table,
                           new_carry.as<int64_t>());
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t2.end("records stream: rows, carry"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    r->n_out = n_out;
    r->out_samples = out_samples;
    r->n_keep = n_keep;
    r->keep_samples = keep_samples;
    r->flip = n_keep > 0;
    return WFA_OK;
}

}  // namespace
}  // namespace wfa

using namespace wfa;

static int use_device_ht(wfa_ctx* c) {
    if (!c) return fail(WFA_E_INVALID, "ctx is null");
    WFA_HIP_CHECK(hipSetDevice(c->device));
    return WFA_OK;
}

extern "C" {

int wfa_hit_rows_source(wfa_ctx* c, int which) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (which != 1 && which != 2) return fail(WFA_E_INVALID, "row source must be 1 (last hit pass) or 2 (last gather)");
    c->ht_src = which;
    return WFA_OK;
}

int wfa_group_hit_windows_count(wfa_ctx* c, int64_t n, const int64_t* timestamp, const int64_t* position,
                                const int32_t* sample_start, const int32_t* sample_end, const int32_t* dt,
                                const int16_t* board, const int16_t* channel, const int64_t* record_id,
                                const double* abs_start_fix, const double* abs_end_fix, double time_window_ns,
                                int64_t* n_events) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || !n_events) return fail(WFA_E_INVALID, "bad arguments");
    if (time_window_ns < 0) return fail(WFA_E_INVALID, "time_window_ns must be >= 0");
    c->ht_n = -1;
    if (n == 0) { c->ht_n = 0; c->ht_groups = 0; c->ht_kind = 1; *n_events = 0; return WFA_OK; }
    if (n > 0x7fffffffLL) return fail(WFA_E_LIMIT, "hit table has %lld rows; the device stages handle < 2^31", (long long)n);
    HitCols h{};
    const bool resident = !timestamp && !position && !sample_start && !sample_end && !dt && !board && !channel && !record_id;
    if (resident) {  // every column NULL: the device-resident rows (wfa_hit_rows_source); sample window = edge_start / edge_end
        if ((rc = resident_cols(c, n, &h))) return rc;
    } else {
        if (!timestamp || !position || !sample_start || !sample_end || !dt || !board || !channel || !record_id)
            return fail(WFA_E_INVALID, "null column");
        if ((rc = upload_cols(c, n, timestamp, position, sample_start, sample_end, dt, board, channel, record_id, &h))) return rc;
    }
    if ((abs_start_fix == nullptr) != (abs_end_fix == nullptr)) return fail(WFA_E_INVALID, "pass both abs_*_fix arrays or neither");
    double *fix0 = nullptr, *fix1 = nullptr;
    if (abs_start_fix && ((rc = upload(c, S_OUT6, abs_start_fix, n, &fix0)) || (rc = upload(c, S_OUT7, abs_end_fix, n, &fix1)))) return rc;
    int64_t n_ev = 0;
    int64_t* perm = nullptr;
    if ((rc = group_cols(c, n, h, fix0, fix1, time_window_ns, &n_ev, &perm, nullptr))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ht_n = n; c->ht_groups = n_ev; c->ht_kind = 1; c->ht_perm = perm;
    *n_events = n_ev;
    return WFA_OK;
}

int wfa_group_hit_windows_fill(wfa_ctx* c, int64_t n, int64_t n_events, int64_t* order, int64_t* event_start,
                               int64_t* t_min, int64_t* t_max) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->ht_n < 0 || c->ht_kind != 1) return fail(WFA_E_STATE, "no event grouping pass has been run");
    if (n != c->ht_n || n_events != c->ht_groups)
        return fail(WFA_E_INVALID, "caller expects %lld hits / %lld events, the pass produced %lld / %lld", (long long)n,
                    (long long)n_events, (long long)c->ht_n, (long long)c->ht_groups);
    if (!event_start) return fail(WFA_E_INVALID, "event_start is null");
    if (n == 0) { event_start[0] = 0; return WFA_OK; }
    if (!order || !t_min || !t_max) return fail(WFA_E_INVALID, "null output");
    WFA_HIP_CHECK(hipMemcpyAsync(order, c->ht_perm, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(event_start, c->ht[S_OUT0].ptr, (size_t)(n_events + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(t_min, c->ht[S_OUT1].ptr, (size_t)n_events * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(t_max, c->ht[S_OUT2].ptr, (size_t)n_events * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_group_multi_channel_count(wfa_ctx* c, int64_t n, const int64_t* timestamp, const int64_t* channel,
                                  double time_window_ps, int64_t* n_events) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || !n_events) return fail(WFA_E_INVALID, "bad arguments");
    c->ht_n = -1;
    if (n == 0) { c->ht_n = 0; c->ht_groups = 0; c->ht_kind = 3; *n_events = 0; return WFA_OK; }
    if (!timestamp || !channel) return fail(WFA_E_INVALID, "null column");
    if (n >= 0x7fffffffLL) return fail(WFA_E_LIMIT, "hit table has %lld rows; the device stages handle < 2^31 - 1", (long long)n);
    int levels = 1;
    while ((1ll << levels) < n) ++levels;  // next^(2^levels) of any hit is n
    int64_t *ts, *ch, *mark, *incl;
    uint64_t *k_ts, *k_ch, *k_ev;
    double* ts_f;
    int32_t* jump;  // two levels, J_k and J_(k+1), used in turn
    if ((rc = upload(c, S_TS, timestamp, n, &ts)) || (rc = upload(c, S_POS, channel, n, &ch)) ||
        (rc = slot(c, S_K0, n, &k_ts)) || (rc = slot(c, S_K1, n, &k_ch)) || (rc = slot(c, S_K2, n, &k_ev)) ||
        (rc = slot(c, S_ABS0, n, &ts_f)) || (rc = slot(c, S_FLAG, n, &mark)) || (rc = slot(c, S_ID, n, &incl)) ||
        (rc = slot(c, S_OUT3, 2 * (n + 1), &jump)))
        return rc;
    LaunchTimer t(c);
    hipLaunchKernelGGL(k_mc_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, ts, ch, k_ts, k_ch);
    int64_t* perm = nullptr;
    {
        const uint64_t* keys[1] = {k_ts};  // df.sort_values("timestamp"), stable
        if ((rc = lexsort(c, n, keys, 1, &perm))) return rc;
    }
    hipLaunchKernelGGL(k_mc_sorted_ts, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, ts, perm, ts_f);
    hipLaunchKernelGGL(k_mc_next, dim3(blocks_for(n + 1)), dim3(kTB), 0, c->stream, n, ts_f, time_window_ps, jump);
    WFA_HIP_CHECK(hipMemsetAsync(mark, 0, (size_t)n * sizeof(int64_t), c->stream));
    const int64_t one = 1;
    WFA_HIP_CHECK(hipMemcpyAsync(mark, &one, sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < levels; ++k)
        hipLaunchKernelGGL(k_mc_mark_jump, dim3(blocks_for(n + 1)), dim3(kTB), 0, c->stream, n, jump + (int64_t)(k & 1) * (n + 1),
                           jump + (int64_t)((k + 1) & 1) * (n + 1), mark);
    size_t tb = 0;
    WFA_HIP_CHECK(rocprim::inclusive_scan(nullptr, tb, mark, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    if ((rc = c->ht[S_CUB].ensure(tb))) return rc;
    tb = c->ht[S_CUB].cap;
    WFA_HIP_CHECK(rocprim::inclusive_scan(c->ht[S_CUB].ptr, tb, mark, incl, (size_t)n, rocprim::plus<int64_t>(), c->stream));
    int64_t n_ev = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&n_ev, incl + (n - 1), sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    hipLaunchKernelGGL(k_event_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, perm, incl, k_ev);
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));  // (`one` and n_ev live on this stack frame)
    int64_t* bounds;
    if ((rc = slot(c, S_OUT0, n_ev + 1, &bounds))) return rc;
    hipLaunchKernelGGL(k_mc_bounds, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, mark, incl, n_ev, bounds);
    {
        // inside a cluster by channel, equal channels in timestamp order: np.lexsort((arange, channel, event)) of the sorted
        // table = a stable sort of the timestamp order by (event, channel)
        const uint64_t* keys[2] = {k_ev, k_ch};
        if ((rc = lexsort(c, n, keys, 2, &perm, perm))) return rc;
    }
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("hit table: group_multi_channel_hits (sort + pointer jumping)"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ht_n = n; c->ht_groups = n_ev; c->ht_kind = 3; c->ht_perm = perm;
    *n_events = n_ev;
    return WFA_OK;
}

int wfa_group_multi_channel_fill(wfa_ctx* c, int64_t n, int64_t n_events, int64_t* order, int64_t* bounds) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->ht_n < 0 || c->ht_kind != 3) return fail(WFA_E_STATE, "no multi-channel grouping pass has been run");
    if (n != c->ht_n || n_events != c->ht_groups)
        return fail(WFA_E_INVALID, "caller expects %lld hits / %lld events, the pass produced %lld / %lld", (long long)n,
                    (long long)n_events, (long long)c->ht_n, (long long)c->ht_groups);
    if (!bounds) return fail(WFA_E_INVALID, "bounds is null");
    if (n == 0) { bounds[0] = 0; return WFA_OK; }
    if (!order) return fail(WFA_E_INVALID, "order is null");
    WFA_HIP_CHECK(hipMemcpyAsync(order, c->ht_perm, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(bounds, c->ht[S_OUT0].ptr, (size_t)(n_events + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_hit_merge_count(wfa_ctx* c, int64_t n, const int64_t* timestamp, const int64_t* position,
                        const int32_t* edge_start, const int32_t* edge_end, const int32_t* dt, const int16_t* board,
                        const int16_t* channel, double merge_gap_ns, double max_total_width_ns, int64_t* n_clusters) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || !n_clusters) return fail(WFA_E_INVALID, "bad arguments");
    c->ht_n = -1;
    if (n == 0) { c->ht_n = 0; c->ht_groups = 0; c->ht_kind = 2; *n_clusters = 0; return WFA_OK; }
    if (n > 0x7fffffffLL) return fail(WFA_E_LIMIT, "hit table has %lld rows; the device stages handle < 2^31", (long long)n);
    HitCols h{};
    const bool resident = !timestamp && !position && !edge_start && !edge_end && !dt && !board && !channel;
    if (resident) {  // every column NULL: the device-resident rows (wfa_hit_rows_source)
        if ((rc = resident_cols(c, n, &h))) return rc;
    } else {
        if (!timestamp || !position || !edge_start || !edge_end || !dt || !board || !channel)
            return fail(WFA_E_INVALID, "null column");
        if ((rc = upload_cols(c, n, timestamp, position, edge_start, edge_end, dt, board, channel, timestamp, &h))) return rc;
    }
    int64_t n_cl = 0;
    int64_t* perm = nullptr;
    if ((rc = merge_cols(c, n, h, merge_gap_ns, max_total_width_ns, &n_cl, &perm))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ht_n = n; c->ht_groups = n_cl; c->ht_kind = 2; c->ht_perm = perm;
    *n_clusters = n_cl;
    return WFA_OK;
}

int wfa_hit_merge_fill(wfa_ctx* c, int64_t n, int64_t n_clusters, int64_t* order, int64_t* cluster_offset) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->ht_n < 0 || c->ht_kind != 2) return fail(WFA_E_STATE, "no hit merge pass has been run");
    if (n != c->ht_n || n_clusters != c->ht_groups)
        return fail(WFA_E_INVALID, "caller expects %lld hits / %lld clusters, the pass produced %lld / %lld", (long long)n,
                    (long long)n_clusters, (long long)c->ht_n, (long long)c->ht_groups);
    if (!cluster_offset) return fail(WFA_E_INVALID, "cluster_offset is null");
    if (n == 0) { cluster_offset[0] = 0; return WFA_OK; }
    if (!order) return fail(WFA_E_INVALID, "order is null");
    WFA_HIP_CHECK(hipMemcpyAsync(order, c->ht_perm, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(cluster_offset, c->ht[S_OUT0].ptr, (size_t)(n_clusters + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_hit_merge_emit(wfa_ctx* c, int64_t n, const int64_t* timestamp, const int32_t* sample_start,
                       const int32_t* sample_end, const int64_t* record_id, const float* height, const float* integral,
                       int64_t n_members, const int64_t* member_hit, int64_t n_clusters, const int64_t* cluster_offset,
                       int64_t* anchor, float* out_height, float* out_integral, int32_t* out_start, int32_t* out_end,
                       float* out_width) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || n_members < 0 || n_clusters < 0) return fail(WFA_E_INVALID, "negative size");
    if (n_clusters == 0) return WFA_OK;
    if (!timestamp || !sample_start || !sample_end || !record_id || !height || !integral || !member_hit || !cluster_offset ||
        !anchor || !out_height || !out_integral || !out_start || !out_end || !out_width)
        return fail(WFA_E_INVALID, "null argument");
    // membership must be well-formed before a kernel indexes with it
    if (cluster_offset[0] != 0 || cluster_offset[n_clusters] != n_members) return fail(WFA_E_INVALID, "cluster_offset does not span the members");
    for (int64_t k = 0; k < n_clusters; ++k)
        if (cluster_offset[k + 1] <= cluster_offset[k]) return fail(WFA_E_INVALID, "empty or unordered cluster %lld", (long long)k);
    for (int64_t j = 0; j < n_members; ++j)
        if (member_hit[j] < 0 || member_hit[j] >= n) return fail(WFA_E_INVALID, "hit index %lld out of range", (long long)member_hit[j]);
    HitCols h{};
    int64_t *d_ts, *d_rid, *d_m, *d_off, *d_anchor;
    int32_t *d_s, *d_e, *o_s, *o_e;
    float *d_h, *d_i, *o_h, *o_i, *o_w;
    if ((rc = upload(c, S_TS, timestamp, n, &d_ts)) || (rc = upload(c, S_START, sample_start, n, &d_s)) ||
        (rc = upload(c, S_END, sample_end, n, &d_e)) || (rc = upload(c, S_RID, record_id, n, &d_rid)) ||
        (rc = upload(c, S_HEIGHT, height, n, &d_h)) || (rc = upload(c, S_INTEGRAL, integral, n, &d_i)) ||
        (rc = upload(c, S_PERM0, member_hit, n_members, &d_m)) || (rc = upload(c, S_OUT0, cluster_offset, n_clusters + 1, &d_off)))
        return rc;
    if ((rc = slot(c, S_OUT1, n_clusters, &d_anchor)) || (rc = slot(c, S_OUT2, n_clusters, &o_h)) || (rc = slot(c, S_OUT3, n_clusters, &o_i)) ||
        (rc = slot(c, S_OUT4, n_clusters, &o_s)) || (rc = slot(c, S_OUT5, n_clusters, &o_e)) || (rc = slot(c, S_OUT6, n_clusters, &o_w)))
        return rc;
    h.ts = d_ts; h.s = d_s; h.e = d_e; h.rid = d_rid;
    c->ht_n = -1;
    LaunchTimer t(c);
    hipLaunchKernelGGL(k_merge_emit, dim3(blocks_for(n_clusters)), dim3(kTB), 0, c->stream, n_clusters, d_off, d_m, h, d_h, d_i,
                       d_anchor, o_h, o_i, o_s, o_e, o_w);
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("hit table: hit_merge emit"))) return rc;
    const size_t m = (size_t)n_clusters;
    WFA_HIP_CHECK(hipMemcpyAsync(anchor, d_anchor, m * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(out_height, o_h, m * 4, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(out_integral, o_i, m * 4, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(out_start, o_s, m * 4, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(out_end, o_e, m * 4, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(out_width, o_w, m * 4, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_records_sort(wfa_ctx* c, int64_t n, const int64_t* timestamp, const int32_t* pid, const int16_t* board,
                     const int16_t* channel, int64_t* order) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0) return fail(WFA_E_INVALID, "negative size");
    if (n == 0) return WFA_OK;
    if (!timestamp || !pid || !board || !channel || !order) return fail(WFA_E_INVALID, "null argument");
    int64_t* d_ts;
    int32_t* d_pid;
    int16_t *d_b, *d_c;
    uint64_t *k_ts, *k_pid, *k_bc;
    if ((rc = upload(c, S_TS, timestamp, n, &d_ts)) || (rc = upload(c, S_DT, pid, n, &d_pid)) ||
        (rc = upload(c, S_BOARD, board, n, &d_b)) || (rc = upload(c, S_CHAN, channel, n, &d_c)) ||
        (rc = slot(c, S_K0, n, &k_ts)) || (rc = slot(c, S_K1, n, &k_pid)) || (rc = slot(c, S_K2, n, &k_bc)))
        return rc;
    c->ht_n = -1;
    LaunchTimer t(c);
    hipLaunchKernelGGL(k_record_keys, dim3(blocks_for(n)), dim3(kTB), 0, c->stream, n, d_ts, d_pid, d_b, d_c, k_ts, k_pid, k_bc);
    int64_t* perm = nullptr;
    const uint64_t* keys[3] = {k_ts, k_pid, k_bc};  // np.lexsort((seq, channel, board, pid, timestamp)); seq = stability
    if ((rc = lexsort(c, n, keys, 3, &perm))) return rc;
    if ((rc = t.end("records: global sort order"))) return rc;
    WFA_HIP_CHECK(hipMemcpyAsync(order, perm, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

// ---- event stream -----------------------------------------------------------------------------------------------------
int wfa_event_stream_begin(wfa_ctx* c, double time_window_ns) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (time_window_ns < 0) return fail(WFA_E_INVALID, "time_window_ns must be >= 0");
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->es.restart();
    c->es.open = true;
    c->es.window_ns = time_window_ns;
    c->es.horizon = -HUGE_VAL;
    return WFA_OK;
}

int wfa_event_stream_push(wfa_ctx* c, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_out_rows,
                          int64_t* n_out_events, int64_t* n_carry) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::EventStream& es = c->es;
    if ((rc = push_checks(es.open, "event", "wfa_event_stream_begin", &es.out_rows,
                          n_rows >= 0 && (n_rows == 0 || hit_rows) && n_out_rows && n_out_events && n_carry, horizon_ps,
                          es.horizon, es.carry.n, n_rows)))
        return rc;
    GroupStepOut r;
    if (es.carry.n + n_rows > 0 &&  // (nothing carried, nothing pushed: no launch)
        ((rc = es.carry.reserve(c, n_rows)) || (rc = es.carry.upload(c, hit_rows, n_rows)) ||
         (rc = group_step<15, 15>(c, es, n_rows, horizon_ps, &r))))
        return rc;
    group_commit(es, r, horizon_ps);
    *n_out_rows = r.n_out;
    *n_out_events = r.n_closed;
    *n_carry = r.n_keep;
    return WFA_OK;
}

int wfa_event_stream_fill(wfa_ctx* c, void* out_rows, int64_t n_out_rows) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!c->es.open || c->es.out_rows < 0) return fail(WFA_E_STATE, "no event stream push has been made");
    if (n_out_rows != c->es.out_rows)
        return fail(WFA_E_INVALID, "caller expects %lld rows, the last push closed %lld", (long long)n_out_rows,
                    (long long)c->es.out_rows);
    if (n_out_rows == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    if ((rc = stream_d2h(c, out_rows, c->es.out.ptr, (size_t)n_out_rows * 84))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_event_stream_end(wfa_ctx* c) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->es.release();
    return WFA_OK;
}

// ---- merge stream -----------------------------------------------------------------------------------------------------
int wfa_merge_stream_begin(wfa_ctx* c, double merge_gap_ns, double max_total_width_ns) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!(merge_gap_ns >= 0)) return fail(WFA_E_INVALID, "merge_gap_ns must be >= 0");
    if (!(max_total_width_ns >= 0)) return fail(WFA_E_INVALID, "max_total_width_ns must be >= 0");
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ms.restart();  // (a stream left open starts over: empty carry, index 0; the buffers are reused)
    c->ms.open = true;
    c->ms.gap_ns = merge_gap_ns;
    c->ms.width_ns = max_total_width_ns;
    c->ms.horizon = -HUGE_VAL;
    return WFA_OK;
}

int wfa_merge_stream_push(wfa_ctx* c, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_merged,
                          int64_t* n_components, int64_t* n_carry, double* open_start_ps) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::MergeStream& ms = c->ms;
    if ((rc = push_checks(ms.open, "merge", "wfa_merge_stream_begin", &ms.out_merged,
                          n_rows >= 0 && (n_rows == 0 || hit_rows) && n_merged && n_components && n_carry && open_start_ps,
                          horizon_ps, ms.horizon, ms.carry.n, n_rows)))
        return rc;
    const MergeIo io{&ms.out, 18, 0};
    MergeStepOut r;
    if ((rc = merge_step(c, ms, io, hit_rows, n_rows, horizon_ps, &r))) return rc;
    merge_commit(ms, r, n_rows, horizon_ps);
    *n_merged = r.n_closed;
    *n_components = r.n_comp;
    *n_carry = r.n_keep;
    *open_start_ps = r.open_start;
    return WFA_OK;
}

int wfa_merge_stream_fill(wfa_ctx* c, void* merged_rows, int64_t* hit_index, int64_t n_merged, int64_t n_components) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!c->ms.open || c->ms.out_merged < 0) return fail(WFA_E_STATE, "no merge stream push has been made");
    if (n_merged != c->ms.out_merged || n_components != c->ms.out_components)
        return fail(WFA_E_INVALID, "caller expects %lld rows / %lld components, the last push closed %lld / %lld",
                    (long long)n_merged, (long long)n_components, (long long)c->ms.out_merged, (long long)c->ms.out_components);
    if (n_merged == 0) return WFA_OK;
    if (!merged_rows || !hit_index) return fail(WFA_E_INVALID, "null output");
    if ((rc = stream_d2h(c, merged_rows, c->ms.out.ptr, (size_t)n_merged * 72)) ||
        (rc = stream_d2h(c, hit_index, c->ms.out_index.ptr, (size_t)n_components * 8)))
        return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_merge_stream_end(wfa_ctx* c) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ms.release();
    return WFA_OK;
}

// ---- merged-event stream ----------------------------------------------------------------------------------------------
int wfa_merged_event_stream_begin(wfa_ctx* c, double merge_gap_ns, double max_total_width_ns, double time_window_ns,
                                  double horizon_margin_ps) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!(merge_gap_ns >= 0)) return fail(WFA_E_INVALID, "merge_gap_ns must be >= 0");
    if (!(max_total_width_ns >= 0)) return fail(WFA_E_INVALID, "max_total_width_ns must be >= 0");
    if (!(time_window_ns >= 0)) return fail(WFA_E_INVALID, "time_window_ns must be >= 0");
    if (!(horizon_margin_ps >= 0) || horizon_margin_ps == HUGE_VAL)
        return fail(WFA_E_INVALID, "horizon_margin_ps must be >= 0 and finite");
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->mes.restart();  // (a stream left open starts over: empty carries, ids 0; the buffers are reused)
    c->mes.open = true;
    c->mes.margin_ps = horizon_margin_ps;
    c->mes.m.gap_ns = merge_gap_ns;
    c->mes.m.width_ns = max_total_width_ns;
    c->mes.m.horizon = -HUGE_VAL;
    c->mes.e.window_ns = time_window_ns;
    c->mes.e.horizon = -HUGE_VAL;
    return WFA_OK;
}

int wfa_merged_event_stream_push(wfa_ctx* c, const void* hit_rows, int64_t n_rows, double horizon_ps, int64_t* n_out_rows,
                                 int64_t* n_out_events, int64_t* n_clusters, int64_t* n_components, int64_t* n_merge_carry,
                                 int64_t* n_event_carry, double* group_horizon_ps) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::MergedEventStream& st = c->mes;
    if ((rc = push_checks(st.open, "merged-event", "wfa_merged_event_stream_begin", &st.e.out_rows,
                          n_rows >= 0 && (n_rows == 0 || hit_rows) && n_out_rows && n_out_events && n_clusters &&
                              n_components && n_merge_carry && n_event_carry && group_horizon_ps,
                          horizon_ps, st.m.horizon, st.m.carry.n, n_rows)))
        return rc;
    // 1. the merge step; its rows go behind the event carry as 88-byte entries, with their fix windows
    const MergeIo io{&st.e.carry.table(), 22, st.e.carry.n};
    MergeStepOut m;
    if ((rc = merge_step(c, st.m, io, hit_rows, n_rows, horizon_ps, &m))) return rc;
    // 2. the grouping horizon: no merged row still to come starts below min(H, open_start'), nor below an earlier G
    double open = m.open_start;
    if (st.margin_ps > 0 && open != HUGE_VAL) open = nextafter(open - 1.5 * st.margin_ps, -HUGE_VAL);
    double g = horizon_ps < open ? horizon_ps : open;
    if (g < st.e.horizon) g = st.e.horizon;
    // 3. the group step over event carry ++ the new merged rows
    GroupStepOut e;
    if (st.e.carry.n + m.n_closed > 0 && (rc = group_step<18, 22>(c, st.e, m.n_closed, g, &e))) return rc;
    merge_commit(st.m, m, n_rows, horizon_ps);
    group_commit(st.e, e, g);
    *n_out_rows = e.n_out;
    *n_out_events = e.n_closed;
    *n_clusters = m.n_closed;
    *n_components = m.n_comp;
    *n_merge_carry = m.n_keep;
    *n_event_carry = e.n_keep;
    *group_horizon_ps = g;
    return WFA_OK;
}

int wfa_merged_event_stream_fill(wfa_ctx* c, void* out_rows, int64_t* hit_index, int64_t n_out_rows, int64_t n_components) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    const wfa_ctx::MergedEventStream& st = c->mes;
    if (!st.open || st.e.out_rows < 0) return fail(WFA_E_STATE, "no merged-event stream push has been made");
    if (n_out_rows != st.e.out_rows || n_components != st.m.out_components)
        return fail(WFA_E_INVALID, "caller expects %lld rows / %lld components, the last push closed %lld / %lld",
                    (long long)n_out_rows, (long long)n_components, (long long)st.e.out_rows, (long long)st.m.out_components);
    if ((n_out_rows > 0 && !out_rows) || (n_components > 0 && !hit_index)) return fail(WFA_E_INVALID, "null output");
    if (n_out_rows > 0 && (rc = stream_d2h(c, out_rows, st.e.out.ptr, (size_t)n_out_rows * 96))) return rc;
    if (n_components > 0 && (rc = stream_d2h(c, hit_index, st.m.out_index.ptr, (size_t)n_components * 8))) return rc;
    if (n_out_rows > 0 || n_components > 0) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_merged_event_stream_end(wfa_ctx* c) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->mes.release();
    return WFA_OK;
}

// ---- df_events stream -------------------------------------------------------------------------------------------------
int wfa_df_event_stream_begin(wfa_ctx* c, double time_window_ps) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!(time_window_ps >= 0)) return fail(WFA_E_INVALID, "time_window_ps must be >= 0");
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ds.restart();  // (a stream left open starts over: empty carry, event id 0; the buffers are reused)
    c->ds.open = true;
    c->ds.window_ps = time_window_ps;
    return WFA_OK;
}

int wfa_df_event_stream_push(wfa_ctx* c, const void* rows, int64_t n_rows, int64_t horizon_ts, int final, int64_t* n_out_rows,
                             int64_t* n_out_events, int64_t* n_carry) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::DfEventStream& ds = c->ds;
    if ((rc = push_checks(ds.open, "df_events", "wfa_df_event_stream_begin", &ds.out_rows,
                          n_rows >= 0 && (n_rows == 0 || rows) && n_out_rows && n_out_events && n_carry, horizon_ts, ds.horizon,
                          ds.carry.n, n_rows)))
        return rc;
    GroupStepOut r;
    if ((rc = dfs_step(c, ds, rows, n_rows, horizon_ts, final, &r))) return rc;
    group_commit(ds, r, horizon_ts);
    *n_out_rows = r.n_out;
    *n_out_events = r.n_closed;
    *n_carry = r.n_keep;
    return WFA_OK;
}

int wfa_df_event_stream_fill(wfa_ctx* c, void* out_rows, int64_t n_out_rows) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (!c->ds.open || c->ds.out_rows < 0) return fail(WFA_E_STATE, "no df_events stream push has been made");
    if (n_out_rows != c->ds.out_rows)
        return fail(WFA_E_INVALID, "caller expects %lld rows, the last push closed %lld", (long long)n_out_rows,
                    (long long)c->ds.out_rows);
    if (n_out_rows == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    if ((rc = stream_d2h(c, out_rows, c->ds.out.ptr, (size_t)n_out_rows * 64))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_df_event_stream_end(wfa_ctx* c) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->ds.release();
    return WFA_OK;
}

// ---- records stream ---------------------------------------------------------------------------------------------------
int wfa_records_stream_begin(wfa_ctx* c, int32_t dt_ns) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (dt_ns <= 0) return fail(WFA_E_INVALID, "dt_ns must be > 0, got %d", (int)dt_ns);
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->rs.restart();  // (a stream left open starts over: empty carries, record id 0; the buffers are reused)
    c->rs.open = true;
    c->rs.dt_ns = dt_ns;
    return WFA_OK;
}

int wfa_records_stream_push(wfa_ctx* c, const uint8_t* block, int64_t n_bytes, int64_t n_waves, const int64_t* timestamp_ps,
                            const int64_t* seq, const int64_t* payload_offset, const int32_t* n_samples, const int16_t* board,
                            const int16_t* channel, const uint16_t* baseline, const uint8_t* trunc, int64_t horizon_ps, int final,
                            int64_t* n_out_records, int64_t* n_out_samples, int64_t* n_carry_records, int64_t* n_carry_samples) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::RecordsStream& rs = c->rs;
    const bool cols = timestamp_ps && seq && payload_offset && n_samples && board && channel && baseline && trunc;
    if ((rc = push_checks(rs.open, "records", "wfa_records_stream_begin", &rs.out_records,
                          n_waves >= 0 && n_bytes >= 0 && (n_waves == 0 || cols) && (n_bytes == 0 || block) && n_out_records &&
                              n_out_samples && n_carry_records && n_carry_samples,
                          horizon_ps, rs.horizon, rs.carry.n, n_waves)))
        return rc;
    // every check of the pushed waves is made here, on the host, before anything goes up
    rs.pack.resize((size_t)n_waves * 5);
    for (int64_t k = 0; k < n_waves; ++k) {
        if (timestamp_ps[k] < rs.horizon)
            return fail(WFA_E_INVALID, "wave %lld: timestamp %lld ps lies below the previous push's horizon (%lld ps)", (long long)k,
                        (long long)timestamp_ps[k], (long long)rs.horizon);
        const int64_t len = n_samples[k], at = payload_offset[k];
        if (len < 0 || (len & 1)) return fail(WFA_E_INVALID, "wave %lld: n_samples %lld is negative or odd", (long long)k, (long long)len);
        if (at < 0 || (at & 3) || at > n_bytes || 2 * len > n_bytes - at)
            return fail(WFA_E_INVALID, "wave %lld: payload [%lld, %lld) outside the block of %lld bytes, or not 4-byte aligned",
                        (long long)k, (long long)at, (long long)(at + 2 * len), (long long)n_bytes);
        int64_t* e = &rs.pack[(size_t)k * 5];
        e[0] = timestamp_ps[k];
        e[1] = seq[k];
        e[2] = at >> 1;
        e[3] = (int64_t)((uint64_t)(uint32_t)len | ((uint64_t)(uint16_t)board[k] << 32) | ((uint64_t)(uint16_t)channel[k] << 48));
        e[4] = (int64_t)((uint64_t)baseline[k] | ((uint64_t)(trunc[k] ? 1u : 0u) << 16));
    }
    RecordsStepOut r;
    if ((rc = records_step(c, rs, block, n_bytes, n_waves, horizon_ps, final, &r))) return rc;
    rs.carry.commit(r.n_keep, r.flip);
    if (r.flip) rs.cur_s ^= 1;
    rs.n_samples = r.keep_samples;
    rs.next_record += r.n_out;
    rs.next_sample += r.out_samples;
    rs.horizon = horizon_ps;
    rs.out_records = r.n_out;
    rs.out_samples = r.out_samples;
    *n_out_records = r.n_out;
    *n_out_samples = r.out_samples;
    *n_carry_records = r.n_keep;
    *n_carry_samples = r.keep_samples;
    return WFA_OK;
}

int wfa_records_stream_fill(wfa_ctx* c, void* out_rows, uint16_t* out_pool, int64_t n_out_records, int64_t n_out_samples) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    wfa_ctx::RecordsStream& rs = c->rs;
    if (!rs.open || rs.out_records < 0) return fail(WFA_E_STATE, "no records stream push has been made");
    if (n_out_records != rs.out_records || n_out_samples != rs.out_samples)
        return fail(WFA_E_INVALID, "caller expects %lld records / %lld samples, the last push released %lld / %lld",
                    (long long)n_out_records, (long long)n_out_samples, (long long)rs.out_records, (long long)rs.out_samples);
    if (n_out_records == 0) return WFA_OK;
    if (!out_rows || (n_out_samples > 0 && !out_pool)) return fail(WFA_E_INVALID, "null output");
    if ((rc = stream_d2h(c, out_rows, rs.out_rows.ptr, (size_t)n_out_records * 102))) return rc;
    if (n_out_samples > 0 && (rc = stream_d2h(c, out_pool, rs.out_pool.ptr, (size_t)n_out_samples * 2))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_records_stream_end(wfa_ctx* c) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->rs.release();
    return WFA_OK;
}

}  // extern "C"

// every slice is checked before a kernel indexes with it; offsets of the packed pool are the running sum
static int gather_offsets(int64_t n, const int64_t* src_offset, const int32_t* length, int64_t src_samples,
                          int64_t* out_offset, int64_t out_samples) {
    int64_t cursor = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = length[r] > 0 ? length[r] : 0;
        if (len > 0 && (src_offset[r] < 0 || src_offset[r] + len > src_samples))
            return fail(WFA_E_INVALID, "record %lld: slice [%lld, %lld) outside the source pool of %lld samples", (long long)r,
                        (long long)src_offset[r], (long long)(src_offset[r] + len), (long long)src_samples);
        out_offset[r] = cursor;
        cursor += len;
    }
    if (cursor != out_samples)
        return fail(WFA_E_INVALID, "lengths add up to %lld samples, caller expects %lld", (long long)cursor, (long long)out_samples);
    return WFA_OK;
}

// k_pool_gather from the device samples d_src into the resident pool (slices already checked by gather_offsets)
static int gather_run(wfa_ctx* c, int64_t n, const int64_t* src_offset, const int32_t* length, const uint16_t* d_src,
                      const int64_t* out_offset, uint16_t* out_pool, int64_t out_samples) {
    int rc;
    int64_t *d_so, *d_do;
    int32_t* d_len;
    if ((rc = upload(c, S_K0, src_offset, n, &d_so)) ||
        (rc = upload(c, S_K1, out_offset, n, &d_do)) || (rc = upload(c, S_K2, length, n, &d_len)))
        return rc;
    if ((rc = c->pool_u16.ensure((size_t)(out_samples > 0 ? out_samples : 1) * sizeof(uint16_t)))) return rc;
    {
        LaunchTimer t(c);
        if (n > 0)
            hipLaunchKernelGGL(k_pool_gather, dim3((unsigned)n), dim3(128), 0, c->stream, n, d_so, d_do, d_len, d_src,
                               c->pool_u16.as<uint16_t>());
        WFA_HIP_CHECK(hipGetLastError());
        if ((rc = t.end("k_pool_gather"))) return rc;
    }
    if (out_pool && out_samples > 0)
        WFA_HIP_CHECK(hipMemcpyAsync(out_pool, c->pool_u16.ptr, (size_t)out_samples * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    // the packed pool is now the resident wave_pool
    pool_replaced(c, out_samples, true);
    return WFA_OK;
}

extern "C" {

int wfa_pool_gather(wfa_ctx* c, int64_t n, const int64_t* src_offset, const int32_t* length, const uint16_t* src_pool,
                    int64_t src_samples, int64_t* out_offset, uint16_t* out_pool, int64_t out_samples) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || src_samples < 0 || out_samples < 0) return fail(WFA_E_INVALID, "negative size");
    if (n > 0 && (!src_offset || !length || !out_offset)) return fail(WFA_E_INVALID, "null argument");
    const bool from_csv = !src_pool && src_samples > 0;  // the samples the last wfa_csv_decode_fill left on the device
    if (from_csv && (!c->csv_filled || c->csv_samples != src_samples))
        return fail(WFA_E_INVALID, "src_pool is null and no decoded CSV samples of that size are resident");
    if ((rc = gather_offsets(n, src_offset, length, src_samples, out_offset, out_samples))) return rc;
    uint16_t* d_src;
    if (from_csv) d_src = c->ht[S_CSV].as<uint16_t>();
    else if ((rc = upload(c, S_F0, src_pool, src_samples, &d_src))) return rc;
    return gather_run(c, n, src_offset, length, d_src, out_offset, out_pool, out_samples);
}

int wfa_csv_arena_gather(wfa_ctx* c, int64_t n, const int64_t* src_offset, const int32_t* length, int64_t* out_offset,
                         uint16_t* out_pool, int64_t out_samples) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || out_samples < 0) return fail(WFA_E_INVALID, "negative size");
    if (n > 0 && (!src_offset || !length || !out_offset)) return fail(WFA_E_INVALID, "null argument");
    if ((rc = gather_offsets(n, src_offset, length, c->arena_filled, out_offset, out_samples))) return rc;
    return gather_run(c, n, src_offset, length, c->csv_arena.as<uint16_t>(), out_offset, out_pool, out_samples);
}

// Host-only: header walk of a CAEN V1725 DAW_DEMO binary stream (utils/formats/v1725.py:66-114).  The stream is a
// chain of variable-length events, so the walk is sequential; it touches 16 + 12 bytes per wave and leaves the
// payloads where they are -- wfa_pool_gather moves them on the GPU.
int wfa_v1725_index(const uint8_t* buf, int64_t n_bytes, int64_t capacity, int16_t* channel, int64_t* timestamp,
                    uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset, int32_t* n_samples, int64_t* n_waves) {
    if (n_bytes < 0 || capacity < 0 || !n_waves || (n_bytes > 0 && !buf)) return fail(WFA_E_INVALID, "bad arguments");
    if (capacity > 0 && (!channel || !timestamp || !trunc || !baseline || !payload_offset || !n_samples))
        return fail(WFA_E_INVALID, "null output column");
    char err[160];
    if (host::v1725_index(buf, n_bytes, capacity, channel, timestamp, trunc, baseline, payload_offset, n_samples, n_waves, err,
                          sizeof(err)))
        return fail(WFA_E_INVALID, "%s", err);
    return WFA_OK;
}

int wfa_v1725_index_block(const uint8_t* buf, int64_t n_bytes, int at_file_end, int64_t capacity, int16_t* channel,
                          int64_t* timestamp, uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset, int32_t* n_samples,
                          int64_t* n_waves, int64_t* consumed_bytes) {
    if (n_bytes < 0 || capacity < 0 || !n_waves || !consumed_bytes || (n_bytes > 0 && !buf))
        return fail(WFA_E_INVALID, "bad arguments");
    if (capacity > 0 && (!channel || !timestamp || !trunc || !baseline || !payload_offset || !n_samples))
        return fail(WFA_E_INVALID, "null output column");
    char err[160];
    if (host::v1725_index_block(buf, n_bytes, at_file_end != 0, capacity, channel, timestamp, trunc, baseline, payload_offset,
                                n_samples, n_waves, consumed_bytes, err, sizeof(err)))
        return fail(WFA_E_INVALID, "%s", err);
    return WFA_OK;
}

}  // extern "C"

// K15 count pass; staged: the text goes up through the pinned staging ring (arena parts) instead of one pageable copy
static int csv_count(wfa_ctx* c, const uint8_t* text, int64_t n_bytes, int delimiter, int32_t samples_start, bool staged,
                     int64_t* n_rows, int64_t* n_samples) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n_bytes < 0 || !n_rows || !n_samples) return fail(WFA_E_INVALID, "bad arguments");
    if (n_bytes > 0 && !text) return fail(WFA_E_INVALID, "text is null");
    if (delimiter <= 0 || delimiter > 127 || delimiter == '\n' || delimiter == '\r' || (delimiter >= '0' && delimiter <= '9') ||
        delimiter == '-' || delimiter == '+')
        return fail(WFA_E_INVALID, "delimiter must be an ASCII character that is not a digit, a sign or a line end");
    if (samples_start < 0) return fail(WFA_E_INVALID, "samples_start must be >= 0");
    if (n_bytes > 0x7fffffff) return fail(WFA_E_LIMIT, "text of %lld bytes; one decode call handles < 2^31 bytes", (long long)n_bytes);
    c->csv_rows = -1; c->csv_samples = -1; c->csv_filled = false;
    *n_rows = 0; *n_samples = 0;
    if (n_bytes == 0) { c->csv_rows = 0; c->csv_samples = 0; c->csv_bytes = 0; return WFA_OK; }
    uint8_t* d_text;
    if ((rc = slot<uint8_t>(c, S_ABS0, n_bytes + 2 * kCsvTile, &d_text))) return rc;
    if (staged) {
        if ((rc = h2d_copy(c, d_text, text, (size_t)n_bytes))) return rc;
    } else {
        WFA_HIP_CHECK(hipMemcpyAsync(d_text, text, (size_t)n_bytes, hipMemcpyHostToDevice, c->stream));
    }
    WFA_HIP_CHECK(hipMemsetAsync(d_text + n_bytes, 0, 2 * kCsvTile, c->stream));  // tiles read past the last row
    const int64_t nb = (n_bytes + kCsvNlBlock * 16 - 1) / (kCsvNlBlock * 16);
    int64_t *d_bc, *d_bs;
    if ((rc = slot<int64_t>(c, S_OUT2, nb, &d_bc)) || (rc = slot<int64_t>(c, S_OUT3, nb, &d_bs))) return rc;
    LaunchTimer t(c);
    hipLaunchKernelGGL((k_csv_newlines<false>), dim3((unsigned)nb), dim3(kCsvNlBlock), 0, c->stream, n_bytes, d_text,
                       (const int64_t*)nullptr, d_bc, (int64_t*)nullptr);
    size_t tmp = 0;
    WFA_HIP_CHECK(rocprim::exclusive_scan(nullptr, tmp, d_bc, d_bs, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), c->stream));
    if ((rc = c->ht[S_CUB].ensure(tmp))) return rc;
    WFA_HIP_CHECK(rocprim::exclusive_scan(c->ht[S_CUB].ptr, tmp, d_bc, d_bs, (int64_t)0, (size_t)nb, rocprim::plus<int64_t>(), c->stream));
    int64_t last[2] = {0, 0};
    WFA_HIP_CHECK(hipMemcpyAsync(&last[0], d_bs + nb - 1, 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(&last[1], d_bc + nb - 1, 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int64_t n_nl = last[0] + last[1];
    int64_t* d_nl;
    if ((rc = slot<int64_t>(c, S_K0, n_nl, &d_nl))) return rc;
    hipLaunchKernelGGL((k_csv_newlines<true>), dim3((unsigned)nb), dim3(kCsvNlBlock), 0, c->stream, n_bytes, d_text,
                       (const int64_t*)d_bs, (int64_t*)nullptr, d_nl);
    const int64_t n_lines = n_nl + (text[n_bytes - 1] != '\n' ? 1 : 0);
    int64_t *d_rs, *d_re, *d_ns, *d_so;
    int32_t* d_nf;
    if ((rc = slot<int64_t>(c, S_K1, n_lines, &d_rs)) || (rc = slot<int64_t>(c, S_K2, n_lines, &d_re)) ||
        (rc = slot<int32_t>(c, S_OUT0, n_lines, &d_nf)) || (rc = slot<int64_t>(c, S_K3, n_lines, &d_ns)) ||
        (rc = slot<int64_t>(c, S_K4, n_lines + 1, &d_so)))
        return rc;
    if (n_lines > 0) {
        hipLaunchKernelGGL(k_csv_lines, dim3(blocks_for(n_lines)), dim3(kTB), 0, c->stream, n_lines, n_nl, n_bytes, d_text,
                           d_nl, d_rs, d_re);
        hipLaunchKernelGGL(k_csv_count, dim3((unsigned)n_lines), dim3(64), 0, c->stream, n_lines, d_text, d_rs, d_re,
                           (uint8_t)delimiter, samples_start, d_nf, d_ns);
        size_t tb = 0;
        WFA_HIP_CHECK(rocprim::exclusive_scan(nullptr, tb, d_ns, d_so, (int64_t)0, (size_t)n_lines, rocprim::plus<int64_t>(), c->stream));
        if ((rc = c->ht[S_CUB].ensure(tb))) return rc;
        WFA_HIP_CHECK(rocprim::exclusive_scan(c->ht[S_CUB].ptr, tb, d_ns, d_so, (int64_t)0, (size_t)n_lines, rocprim::plus<int64_t>(), c->stream));
    }
    WFA_HIP_CHECK(hipGetLastError());
    if ((rc = t.end("csv: index rows + count fields"))) return rc;
    int64_t last_off = 0, last_n = 0;
    if (n_lines > 0) {
        WFA_HIP_CHECK(hipMemcpyAsync(&last_off, d_so + n_lines - 1, 8, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipMemcpyAsync(&last_n, d_ns + n_lines - 1, 8, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    }
    c->csv_rows = n_lines; c->csv_samples = last_off + last_n; c->csv_bytes = n_bytes;
    c->csv_samples_start = samples_start; c->csv_delim = delimiter;
    *n_rows = n_lines; *n_samples = c->csv_samples;
    return WFA_OK;
}

// K15 fill pass.  arena: the samples go to csv_arena[sample_base + sample_offset[r] ...] (range checked by the caller)
// instead of the S_CSV slot, and sample_offset comes back shifted by sample_base
static int csv_fill(wfa_ctx* c, int64_t n_rows, int32_t n_meta, const int32_t* meta_cols, int64_t* meta, int64_t* row_offset,
                    int32_t* n_fields, int64_t* sample_offset, uint16_t* samples, int64_t n_samples, bool arena,
                    int64_t sample_base) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (c->csv_rows < 0) return fail(WFA_E_STATE, "no wfa_csv_decode_count pass has been run");
    if (n_rows != c->csv_rows || n_samples != c->csv_samples)
        return fail(WFA_E_INVALID, "the count pass found %lld rows / %lld samples", (long long)c->csv_rows, (long long)c->csv_samples);
    if (arena && (sample_base < 0 || sample_base > c->arena_filled ||
                  sample_base + n_samples > (int64_t)(c->csv_arena.cap / sizeof(uint16_t))))
        return fail(WFA_E_INVALID, "arena part [%lld, %lld) outside the reserved %lld samples or past the filled %lld",
                    (long long)sample_base, (long long)(sample_base + n_samples),
                    (long long)(c->csv_arena.cap / sizeof(uint16_t)), (long long)c->arena_filled);
    if (n_meta < 0 || n_meta > kCsvMaxMeta) return fail(WFA_E_INVALID, "n_meta must be 0..%d", kCsvMaxMeta);
    if (n_meta > 0 && (!meta_cols || !meta)) return fail(WFA_E_INVALID, "null meta arguments");
    CsvCols cols{};
    cols.n_meta = n_meta;
    for (int j = 0; j < n_meta; ++j) {
        if (meta_cols[j] < 0 || meta_cols[j] >= c->csv_samples_start)
            return fail(WFA_E_INVALID, "meta column %d is not before samples_start = %d", meta_cols[j], c->csv_samples_start);
        cols.col[j] = meta_cols[j];
    }
    if (n_rows == 0) { c->csv_filled = !arena; return WFA_OK; }
    int64_t* d_meta;
    uint16_t* d_samples = arena ? c->csv_arena.as<uint16_t>() + sample_base : nullptr;
    unsigned long long* d_err;
    if ((rc = slot<int64_t>(c, S_OUT1, n_rows * (n_meta > 0 ? n_meta : 1), &d_meta)) ||
        (!arena && (rc = slot<uint16_t>(c, S_CSV, n_samples, &d_samples))) ||
        (rc = slot<unsigned long long>(c, S_FLAG, 1, &d_err)))
        return rc;
    WFA_HIP_CHECK(hipMemsetAsync(d_err, 0xff, 8, c->stream));
    WFA_HIP_CHECK(hipMemsetAsync(d_meta, 0, (size_t)n_rows * (n_meta > 0 ? n_meta : 1) * 8, c->stream));
    {
        LaunchTimer t(c);
        hipLaunchKernelGGL(k_csv_decode, dim3((unsigned)n_rows), dim3(64), 0, c->stream, n_rows, c->ht[S_ABS0].as<uint8_t>(),
                           c->ht[S_K1].as<int64_t>(), c->ht[S_K2].as<int64_t>(), (uint8_t)c->csv_delim, c->csv_samples_start,
                           cols, c->ht[S_K4].as<int64_t>(), d_meta, d_samples, d_err);
        WFA_HIP_CHECK(hipGetLastError());
        if ((rc = t.end("k_csv_decode"))) return rc;
    }
    unsigned long long err = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, c->stream));
    if (n_meta > 0) WFA_HIP_CHECK(hipMemcpyAsync(meta, d_meta, (size_t)n_rows * n_meta * 8, hipMemcpyDeviceToHost, c->stream));
    if (row_offset) WFA_HIP_CHECK(hipMemcpyAsync(row_offset, c->ht[S_K1].ptr, (size_t)n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    if (n_fields) WFA_HIP_CHECK(hipMemcpyAsync(n_fields, c->ht[S_OUT0].ptr, (size_t)n_rows * 4, hipMemcpyDeviceToHost, c->stream));
    if (sample_offset) WFA_HIP_CHECK(hipMemcpyAsync(sample_offset, c->ht[S_K4].ptr, (size_t)n_rows * 8, hipMemcpyDeviceToHost, c->stream));
    if (samples && n_samples > 0)
        WFA_HIP_CHECK(hipMemcpyAsync(samples, d_samples, (size_t)n_samples * 2, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (err != ~0ull) {
        const long long row = (long long)(err >> 24), field = (long long)((err >> 2) & 0x3fffff);
        if ((err & 3) == kCsvErrRange)
            return fail(WFA_E_INVALID, "row %lld field %lld: sample outside the uint16 range", row, field);
        return fail(WFA_E_INVALID, "row %lld field %lld: not a decimal integer", row, field);
    }
    if (!arena) {
        c->csv_filled = true;
        return WFA_OK;
    }
    if (sample_offset)
        for (int64_t r = 0; r < n_rows; ++r) sample_offset[r] += sample_base;
    c->arena_filled = std::max(c->arena_filled, sample_base + n_samples);
    return WFA_OK;
}

extern "C" {

// K15 entry points: see include/wfa_hip.h
int wfa_csv_decode_count(wfa_ctx* c, const uint8_t* text, int64_t n_bytes, int delimiter, int32_t samples_start,
                         int64_t* n_rows, int64_t* n_samples) {
    return csv_count(c, text, n_bytes, delimiter, samples_start, false, n_rows, n_samples);
}

int wfa_csv_decode_fill(wfa_ctx* c, int64_t n_rows, int32_t n_meta, const int32_t* meta_cols, int64_t* meta,
                        int64_t* row_offset, int32_t* n_fields, int64_t* sample_offset, uint16_t* samples,
                        int64_t n_samples) {
    return csv_fill(c, n_rows, n_meta, meta_cols, meta, row_offset, n_fields, sample_offset, samples, n_samples, false, 0);
}

int wfa_csv_arena_reserve(wfa_ctx* c, int64_t n_samples, int keep_filled) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n_samples < 0) return fail(WFA_E_INVALID, "negative size");
    const size_t bytes = (size_t)(n_samples > 0 ? n_samples : 1) * sizeof(uint16_t);
    if (!keep_filled) c->arena_filled = 0;
    if (bytes <= c->csv_arena.cap) return WFA_OK;
    if (c->arena_filled == 0) return c->csv_arena.ensure(bytes);
    // grow, keeping [0, arena_filled): new buffer, device copy, swap (DevBuf::ensure drops the contents)
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes + 256);
    if (e != hipSuccess) return fail(WFA_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    e = hipMemcpyAsync(p, c->csv_arena.ptr, (size_t)c->arena_filled * sizeof(uint16_t), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(WFA_E_HIP, "arena growth copy failed: %s", hipGetErrorString(e));
    }
    c->csv_arena.release();
    c->csv_arena.ptr = p;
    c->csv_arena.cap = bytes;
    return WFA_OK;
}

int wfa_csv_arena_count(wfa_ctx* c, const uint8_t* text, int64_t n_bytes, int delimiter, int32_t samples_start,
                        int64_t* n_rows, int64_t* n_samples) {
    return csv_count(c, text, n_bytes, delimiter, samples_start, true, n_rows, n_samples);
}

int wfa_csv_arena_fill(wfa_ctx* c, int64_t sample_base, int64_t n_rows, int32_t n_meta, const int32_t* meta_cols,
                       int64_t* meta, int64_t* row_offset, int32_t* n_fields, int64_t* sample_offset, int64_t n_samples) {
    return csv_fill(c, n_rows, n_meta, meta_cols, meta, row_offset, n_fields, sample_offset, nullptr, n_samples, true,
                    sample_base);
}

int wfa_csv_arena_filled(wfa_ctx* c, int64_t* filled, int64_t* capacity) {
    if (!c) return fail(WFA_E_INVALID, "ctx is null");
    if (filled) *filled = c->arena_filled;
    if (capacity) *capacity = (int64_t)(c->csv_arena.cap / sizeof(uint16_t));
    return WFA_OK;
}

}  // extern "C"


// ---- st_waveforms rows (k_st_pack) ----------------------------------------------------------------------------------
namespace {
struct StPackLoop {
    wfa_ctx* c;
    StPackArgs a;
    uint8_t* buf[2];
    int64_t rows_per_batch, n, next;  // next: first row of the batch to pack next
    int launch() {  // pack the batch starting at row `next` into buf[(next / rows_per_batch) & 1]
        if (next >= n) return WFA_OK;
        const int64_t k = next / rows_per_batch;
        a.row0 = next;
        a.n_rows = std::min(rows_per_batch, n - next);
        const uint64_t bytes = (uint64_t)a.n_rows * a.stride;
        a.n_chunks = (uint32_t)((bytes + 15) / 16);
        LaunchTimer t(c, true);
        hipLaunchKernelGGL(k_st_pack, dim3((a.n_chunks + kStBlock - 1) / kStBlock), dim3(kStBlock), 0, c->stream, a,
                           buf[k & 1]);
        WFA_HIP_CHECK(hipGetLastError());
        next += a.n_rows;
        return t.end("k_st_pack");
    }
    static int launch_cb(void* self) { return static_cast<StPackLoop*>(self)->launch(); }
};
}  // namespace

extern "C" {

int wfa_st_pack(wfa_ctx* c, int64_t n, int source, const uint16_t* src_pool, int64_t src_samples,
                const int64_t* src_offset, const int32_t* src_len, int32_t wave_length, const double* baseline,
                const double* baseline_upstream, const int64_t* timestamp, const int64_t* record_id, const int32_t* dt,
                const int32_t* event_length, const int16_t* board, const int16_t* channel, const uint8_t* polarity,
                const uint32_t* polarity_table, int32_t n_polarity, int64_t batch_bytes, uint8_t* out) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n < 0 || src_samples < 0) return fail(WFA_E_INVALID, "negative size");
    if (wave_length < 0 || wave_length > (1 << 28)) return fail(WFA_E_INVALID, "wave_length %d out of range", wave_length);
    if (n_polarity < 1 || n_polarity > kStMaxPol) return fail(WFA_E_INVALID, "1..%d polarity strings", kStMaxPol);
    if (!polarity_table) return fail(WFA_E_INVALID, "null polarity table");
    if (n == 0) return WFA_OK;
    if (!src_offset || !src_len || !baseline || !baseline_upstream || !timestamp || !record_id || !dt || !event_length ||
        !board || !channel || !polarity || !out)
        return fail(WFA_E_INVALID, "null argument");
    const uint16_t* d_src = nullptr;
    switch (source) {
    case WFA_ST_SRC_HOST:
        if (src_samples > 0 && !src_pool) return fail(WFA_E_INVALID, "src_pool is null");
        break;
    case WFA_ST_SRC_CSV:
        if (!c->csv_filled || c->csv_samples != src_samples)
            return fail(WFA_E_INVALID, "no decoded CSV samples of that size are resident");
        d_src = c->ht[S_CSV].as<uint16_t>();
        break;
    case WFA_ST_SRC_ARENA:
        if (src_samples != c->arena_filled)
            return fail(WFA_E_INVALID, "the arena holds %lld samples, not %lld", (long long)c->arena_filled, (long long)src_samples);
        d_src = c->csv_arena.as<uint16_t>();
        break;
    case WFA_ST_SRC_POOL:
        if (!c->have_u16 || c->pool_n != src_samples)
            return fail(WFA_E_INVALID, "the resident wave_pool holds %lld samples, not %lld",
                        (long long)(c->have_u16 ? c->pool_n : 0), (long long)src_samples);
        d_src = c->pool_u16.as<uint16_t>();
        break;
    default:
        return fail(WFA_E_INVALID, "unknown sample source %d", source);
    }
    // every slice a lane may read, and every polarity code, is checked before the launch
    for (int64_t r = 0; r < n; ++r) {
        const int64_t len = std::min<int64_t>(std::max<int32_t>(src_len[r], 0), wave_length);
        if (len > 0 && (src_offset[r] < 0 || src_offset[r] + len > src_samples))
            return fail(WFA_E_INVALID, "row %lld: slice [%lld, %lld) outside the source of %lld samples", (long long)r,
                        (long long)src_offset[r], (long long)(src_offset[r] + len), (long long)src_samples);
        if (polarity[r] >= n_polarity)
            return fail(WFA_E_INVALID, "row %lld: polarity code %d, table has %d strings", (long long)r, polarity[r], n_polarity);
    }
    const uint64_t stride = kStHeader + 2ull * (uint64_t)wave_length;
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(batch_bytes, 1), 1ll << 30);
    const int64_t rows_per_batch = std::min<int64_t>(n, std::max<int64_t>(1, cap / (int64_t)stride));
    const uint64_t buf_bytes = ((uint64_t)rows_per_batch * stride + 15) / 16 * 16;
    if (buf_bytes >= (1ull << 31)) return fail(WFA_E_LIMIT, "row of %llu bytes too long", (unsigned long long)stride);

    StPackArgs a{};
    if (source == WFA_ST_SRC_HOST) {
        uint16_t* d;
        if ((rc = slot<uint16_t>(c, S_F0, src_samples, &d))) return rc;
        if ((rc = h2d_copy(c, d, src_pool, (size_t)src_samples * sizeof(uint16_t)))) return rc;
        d_src = d;
    }
    int64_t *d_off, *d_ts, *d_rid;
    int32_t *d_len, *d_dt, *d_ev;
    double *d_bl, *d_blu;
    int16_t *d_b, *d_ch;
    uint8_t *d_pol, *d_out0, *d_out1;
    uint32_t* d_tab;
    if ((rc = upload(c, S_K0, src_offset, n, &d_off)) || (rc = upload(c, S_K1, src_len, n, &d_len)) ||
        (rc = upload(c, S_HEIGHT, baseline, n, &d_bl)) || (rc = upload(c, S_INTEGRAL, baseline_upstream, n, &d_blu)) ||
        (rc = upload(c, S_TS, timestamp, n, &d_ts)) || (rc = upload(c, S_RID, record_id, n, &d_rid)) ||
        (rc = upload(c, S_DT, dt, n, &d_dt)) || (rc = upload(c, S_K2, event_length, n, &d_ev)) ||
        (rc = upload(c, S_BOARD, board, n, &d_b)) || (rc = upload(c, S_CHAN, channel, n, &d_ch)) ||
        (rc = upload(c, S_ID, polarity, n, &d_pol)) || (rc = upload(c, S_CNT2, polarity_table, (int64_t)n_polarity * 8, &d_tab)) ||
        (rc = slot<uint8_t>(c, S_OUT2, (int64_t)buf_bytes, &d_out0)) ||
        (rc = slot<uint8_t>(c, S_OUT3, n > rows_per_batch ? (int64_t)buf_bytes : 1, &d_out1)))
        return rc;
    a.src = d_src; a.src_off = d_off; a.src_len = d_len; a.baseline = d_bl; a.baseline_up = d_blu; a.ts = d_ts;
    a.rid = d_rid; a.dt = d_dt; a.ev_len = d_ev; a.board = d_b; a.chan = d_ch; a.pol = d_pol; a.pol_tab = d_tab;
    a.stride = (uint32_t)stride;
    a.magic = (uint32_t)(0xffffffffu / (uint32_t)stride);
    a.L = wave_length;
    StPackLoop loop{c, a, {d_out0, d_out1}, rows_per_batch, n, 0};
    if ((rc = loop.launch())) return rc;
    // batch k goes down through the staging ring; batch k + 1 is packed into the other buffer meanwhile
    for (int64_t row = 0; row < n; row += rows_per_batch) {
        const int64_t k = row / rows_per_batch;
        const int64_t rows = std::min(rows_per_batch, n - row);
        if ((rc = d2h_staged(c, out + (uint64_t)row * stride, loop.buf[k & 1], (size_t)((uint64_t)rows * stride),
                             &StPackLoop::launch_cb, &loop)))
            return rc;
    }
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

}  // extern "C"


// ---- RecordsView matrices (k_view_gather) ---------------------------------------------------------------------------
// (reference: core/data/records_view.py:216-330 `_waves_many` / `_signals_many`.)  Output-stationary like k_st_pack: a
// lane owns eight consecutive samples of the batch's flat n_rows x pad_len matrix, finds its (row, column) with a
// reciprocal multiply, reads the eight source samples (uint16: aligned dwords realigned by a funnel shift, only dwords
// holding a sample of this row's window; float32: two 16-byte loads when aligned), applies the row's cast / baseline
// subtraction / sign flip and stores 16-byte vectors; the eight mask bytes go out as one 8-byte store.
namespace {
constexpr int kViewBlock = 256;
constexpr uint32_t kViewRun = 8;  // output samples per lane

struct ViewArgs {
    const void* pool;           // uint16 or float samples of the resident pool
    const int64_t* off;         // resident records columns
    const int32_t* len;
    const double* baseline;
    const int8_t* pol;
    const int64_t* rec_index;   // per row of the whole request
    const double* bl_override;  // per row of the whole request, or null
    int64_t row0;               // first row of this batch
    uint32_t n_rows;            // rows of this batch
    uint32_t n_chunks;          // runs of kViewRun samples in this batch (the buffers are padded to a whole run)
    uint32_t pad_len;
    uint32_t magic;             // floor((2^32 - 1) / pad_len)
    int32_t sample_start, sample_end, mode;
};

struct ViewRow {
    int64_t at;   // first source sample of the window
    int32_t n;    // window length
    double b;
    bool flip;
};

__device__ __forceinline__ ViewRow view_row(const ViewArgs& a, uint32_t r) {
    const int64_t gr = a.row0 + r;
    const int64_t ri = a.rec_index[gr];
    const int32_t L = a.len[ri];
    const int32_t end = min(a.sample_end < 0 ? L : a.sample_end, L);
    const int32_t start = min(max(a.sample_start, 0), end);
    ViewRow v;
    v.at = a.off[ri] + start;
    v.n = end - start;
    v.b = a.bl_override ? a.bl_override[gr] : a.baseline[ri];
    v.flip = a.mode == WFA_VIEW_SIGNALS && a.pol[ri] == WFA_POL_POSITIVE;
    return v;
}

// one output sample: a cast, at most one subtraction, and the sign BIT flipped (0.0 -> -0.0, like numpy's unary minus)
template <typename O>
struct ViewOp {
    O b;
    bool sub, flip;
    __device__ __forceinline__ ViewOp(const ViewRow& row, int mode) : b((O)row.b), sub(mode != WFA_VIEW_WAVES), flip(row.flip) {}
    template <typename S>
    __device__ __forceinline__ O operator()(S x) const {
        if constexpr (sizeof(O) == 2) {
            return (O)x;
        } else if constexpr (sizeof(O) == 4) {
            float v = (float)x;
            if (sub) v = v - b;
            return flip ? __uint_as_float(__float_as_uint(v) ^ 0x80000000u) : v;
        } else {
            double v = (double)x;
            if (sub) v = v - b;
            return flip ? __longlong_as_double(__double_as_longlong(v) ^ (long long)0x8000000000000000ull) : v;
        }
    }
};

// samples [at, at + nv) of the pool into x[0 .. nv); the rest of x is unspecified
__device__ __forceinline__ void view_load8(const uint16_t* pool, int64_t at, int nv, uint16_t (&x)[8]) {
    const uint32_t* p32 = reinterpret_cast<const uint32_t*>(pool);
    const int64_t ab = at >> 1, lim = at + nv;
    const bool odd = at & 1;
    uint32_t d[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)  // only dwords holding a sample of this window are read
        d[i] = (nv > 0 && (i < 4 || odd) && 2 * (ab + i) < lim) ? p32[ab + i] : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t w = odd ? __builtin_amdgcn_alignbit(d[j + 1], d[j], 16) : d[j];
        x[2 * j] = (uint16_t)(w & 0xffffu);
        x[2 * j + 1] = (uint16_t)(w >> 16);
    }
}

__device__ __forceinline__ void view_load8(const float* pool, int64_t at, int nv, float (&x)[8]) {
    if (nv == 8 && (at & 3) == 0) {
        const float4 lo = *reinterpret_cast<const float4*>(pool + at), hi = *reinterpret_cast<const float4*>(pool + at + 4);
        x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w;
        x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = j < nv ? pool[at + j] : 0.f;
    }
}

template <typename S, typename O>
__global__ __launch_bounds__(kViewBlock) void k_view_gather(ViewArgs a, O* __restrict__ out, uint8_t* __restrict__ mask) {
    const uint32_t g = blockIdx.x * kViewBlock + threadIdx.x;
    if (g >= a.n_chunks) return;
    const uint32_t s = g * kViewRun;  // flat sample index in the batch (< 2^31)
    uint32_t r = __umulhi(s, a.magic);  // floor(s / pad_len) or up to two less
    uint32_t p = s - r * a.pad_len;
    if (p >= a.pad_len) { ++r; p -= a.pad_len; }
    if (p >= a.pad_len) { ++r; p -= a.pad_len; }
    const S* pool = static_cast<const S*>(a.pool);
    union {
        O v[kViewRun];
        uint4 q[kViewRun * sizeof(O) / 16];
    } u;
    uint32_t valid = 0;  // bit j: sample j of the run lies in its row's window
    if (p + kViewRun <= a.pad_len) {
        // eight columns of one row (s < n_rows * pad_len, so the row exists)
        const ViewRow row = view_row(a, r);
        const int nv = max(0, min((int)kViewRun, row.n - (int)p));
        S x[kViewRun];
        view_load8(pool, row.at + p, nv, x);
        const ViewOp<O> op(row, a.mode);
#pragma unroll
        for (int j = 0; j < (int)kViewRun; ++j) u.v[j] = j < nv ? op(x[j]) : (O)0;
        valid = (1u << nv) - 1u;
    } else {
        // a row boundary (or several: pad_len < 8) or the padding after the last row: sample by sample
#pragma unroll
        for (int j = 0; j < (int)kViewRun; ++j) {
            O v = (O)0;
            if (r < a.n_rows) {
                const ViewRow row = view_row(a, r);
                if ((int)p < row.n) {
                    v = ViewOp<O>(row, a.mode)(pool[row.at + p]);
                    valid |= 1u << j;
                }
            }
            u.v[j] = v;
            if (++p == a.pad_len) { p = 0; ++r; }
        }
    }
    uint4* o = reinterpret_cast<uint4*>(out + s);
#pragma unroll
    for (int k = 0; k < (int)(kViewRun * sizeof(O) / 16); ++k) o[k] = u.q[k];
    if (mask) {
        // bit i of a nibble -> byte i of a dword (the four partial products never meet, so nothing carries)
        const uint32_t lo = ((valid & 0xfu) * 0x00204081u) & 0x01010101u;
        const uint32_t hi = ((valid >> 4) * 0x00204081u) & 0x01010101u;
        *reinterpret_cast<uint2*>(mask + s) = make_uint2(lo, hi);
    }
}

struct ViewLoop {
    wfa_ctx* c;
    ViewArgs a;
    int source, out_dtype;
    void* buf[2];
    uint8_t* mbuf[2];  // null without a mask
    int64_t rows_per_batch, n, next;  // next: first row of the batch to build next
    template <typename S, typename O>
    void run(int k) {
        hipLaunchKernelGGL((k_view_gather<S, O>), dim3((a.n_chunks + kViewBlock - 1) / kViewBlock), dim3(kViewBlock), 0,
                           c->stream, a, static_cast<O*>(buf[k]), mbuf[k]);
    }
    int launch() {  // build the batch starting at row `next` into buffer (next / rows_per_batch) & 1
        if (next >= n) return WFA_OK;
        const int k = (int)((next / rows_per_batch) & 1);
        a.row0 = next;
        a.n_rows = (uint32_t)std::min(rows_per_batch, n - next);
        a.n_chunks = (uint32_t)(((uint64_t)a.n_rows * a.pad_len + kViewRun - 1) / kViewRun);
        LaunchTimer t(c, true);
        if (source == WFA_SRC_RAW) {
            if (out_dtype == WFA_VIEW_U16) run<uint16_t, uint16_t>(k);
            else if (out_dtype == WFA_VIEW_F32) run<uint16_t, float>(k);
            else run<uint16_t, double>(k);
        } else {
            if (out_dtype == WFA_VIEW_F32) run<float, float>(k);
            else run<float, double>(k);
        }
        WFA_HIP_CHECK(hipGetLastError());
        next += a.n_rows;
        return t.end("k_view_gather");
    }
    static int launch_cb(void* self) { return static_cast<ViewLoop*>(self)->launch(); }
};
}  // namespace

extern "C" {

int wfa_view_gather(wfa_ctx* c, int64_t n_rows, const int64_t* rec_index, int32_t sample_start, int32_t sample_end,
                    int32_t pad_len, int mode, int source, int out_dtype, const double* baseline_override,
                    int64_t batch_bytes, void* out, uint8_t* mask) {
    int rc = use_device_ht(c);
    if (rc) return rc;
    if (n_rows < 0) return fail(WFA_E_INVALID, "negative row count %lld", (long long)n_rows);
    if (pad_len < 0) return fail(WFA_E_INVALID, "negative pad_len %d", pad_len);
    if (mode != WFA_VIEW_WAVES && mode != WFA_VIEW_WAVES_BASELINE && mode != WFA_VIEW_SIGNALS)
        return fail(WFA_E_INVALID, "unknown view mode %d", mode);
    if (source != WFA_SRC_RAW && source != WFA_SRC_F32) return fail(WFA_E_INVALID, "unknown view source %d", source);
    if (out_dtype != WFA_VIEW_U16 && out_dtype != WFA_VIEW_F32 && out_dtype != WFA_VIEW_F64)
        return fail(WFA_E_INVALID, "unknown view output type %d", out_dtype);
    if (out_dtype == WFA_VIEW_U16 && (source != WFA_SRC_RAW || mode != WFA_VIEW_WAVES))
        return fail(WFA_E_INVALID, "uint16 output is a copy: only plain waves of the uint16 pool have it");
    if (!c->have_records) return fail(WFA_E_STATE, "records not uploaded");
    if (source == WFA_SRC_RAW ? !c->have_u16 : !c->have_f32)
        return fail(WFA_E_STATE, source == WFA_SRC_RAW ? "wave_pool (uint16) not uploaded" : "float32 pool not resident");
    if (n_rows > 0 && !rec_index) return fail(WFA_E_INVALID, "rec_index is null");
    const size_t itemsize = out_dtype == WFA_VIEW_U16 ? 2 : out_dtype == WFA_VIEW_F32 ? 4 : 8;
    if (n_rows > 0 && pad_len > 0 && !out) return fail(WFA_E_INVALID, "out is null");
    // the lengths of the resident table, fetched once per records upload: every row is sized and checked on the host
    if (!c->len_host_valid) {
        c->len_host.resize((size_t)c->R);
        if (c->R > 0)
            WFA_HIP_CHECK(hipMemcpyAsync(c->len_host.data(), c->len.ptr, (size_t)c->R * 4, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->len_host_valid = true;
    }
    int64_t max_window = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        if (rec_index[r] < 0 || rec_index[r] >= c->R)
            return fail(WFA_E_INVALID, "row %lld: record index %lld outside the resident table of %lld records", (long long)r,
                        (long long)rec_index[r], (long long)c->R);
        const int32_t L = c->len_host[(size_t)rec_index[r]];
        const int32_t end = std::min(sample_end < 0 ? L : sample_end, L);
        const int32_t start = std::min(std::max<int32_t>(sample_start, 0), end);
        max_window = std::max<int64_t>(max_window, end - start);
    }
    if (pad_len < max_window) return fail(WFA_E_INVALID, "pad_len (%d) < max length (%lld)", pad_len, (long long)max_window);
    if (n_rows == 0 || pad_len == 0) return WFA_OK;
    const uint64_t row_bytes = (uint64_t)pad_len * itemsize;
    if (max_window == 0) {  // nothing to gather
        std::memset(out, 0, (size_t)((uint64_t)n_rows * row_bytes));
        if (mask) std::memset(mask, 0, (size_t)((uint64_t)n_rows * (uint64_t)pad_len));
        return WFA_OK;
    }
    const int64_t cap = std::min<int64_t>(std::max<int64_t>(batch_bytes, 1), 1ll << 30);
    const int64_t rows_per_batch = std::min<int64_t>(n_rows, std::max<int64_t>(1, cap / (int64_t)row_bytes));
    const uint64_t buf_samples = ((uint64_t)rows_per_batch * (uint64_t)pad_len + kViewRun - 1) / kViewRun * kViewRun;
    if (buf_samples >= (1ull << 31)) return fail(WFA_E_LIMIT, "row of %d samples too long", pad_len);

    int64_t* d_idx;
    double* d_bl = nullptr;
    uint8_t *d_out0, *d_out1, *d_m0 = nullptr, *d_m1 = nullptr;
    const bool two = n_rows > rows_per_batch;
    if ((rc = upload(c, S_K0, rec_index, n_rows, &d_idx)) ||
        (baseline_override && (rc = upload(c, S_HEIGHT, baseline_override, n_rows, &d_bl))) ||
        (rc = slot<uint8_t>(c, S_OUT2, (int64_t)(buf_samples * itemsize), &d_out0)) ||
        (rc = slot<uint8_t>(c, S_OUT3, two ? (int64_t)(buf_samples * itemsize) : 1, &d_out1)) ||
        (mask && ((rc = slot<uint8_t>(c, S_OUT4, (int64_t)buf_samples, &d_m0)) ||
                  (rc = slot<uint8_t>(c, S_OUT5, two ? (int64_t)buf_samples : 1, &d_m1)))))
        return rc;
    ViewArgs a{};
    a.pool = source == WFA_SRC_RAW ? c->pool_u16.ptr : c->pool_f32.ptr;
    a.off = c->off.as<int64_t>(); a.len = c->len.as<int32_t>(); a.baseline = c->baseline.as<double>(); a.pol = c->pol.as<int8_t>();
    a.rec_index = d_idx; a.bl_override = d_bl;
    a.pad_len = (uint32_t)pad_len;
    a.magic = 0xffffffffu / (uint32_t)pad_len;
    a.sample_start = sample_start; a.sample_end = sample_end; a.mode = mode;
    ViewLoop loop{c, a, source, out_dtype, {d_out0, d_out1}, {d_m0, d_m1}, rows_per_batch, n_rows, 0};
    if ((rc = loop.launch())) return rc;
    // batch k goes down through the staging ring; batch k + 1 is built into the other buffers meanwhile
    for (int64_t row = 0; row < n_rows; row += rows_per_batch) {
        const int k = (int)((row / rows_per_batch) & 1);
        const uint64_t rows = (uint64_t)std::min(rows_per_batch, n_rows - row);
        if ((rc = d2h_staged(c, static_cast<uint8_t*>(out) + (uint64_t)row * row_bytes, loop.buf[k], (size_t)(rows * row_bytes),
                             &ViewLoop::launch_cb, &loop)))
            return rc;
        if (mask && (rc = d2h_staged(c, mask + (uint64_t)row * (uint64_t)pad_len, loop.mbuf[k], (size_t)(rows * (uint64_t)pad_len),
                                     nullptr, nullptr)))
            return rc;
    }
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

}  // extern "C"
