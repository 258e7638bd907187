// C ABI of libwfa_hip.so (see include/wfa_hip.h): context, resident buffers, kernel calls.

#include <cmath>
#include <cstdlib>
#include <new>

#include <algorithm>
#include <chrono>
#include <thread>

#include "wfa_common.hpp"
#include "wfa_host.hpp"
#include "wfa_kernels.hpp"

namespace wfa {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int DevBuf::ensure(size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (bytes <= cap) return WFA_OK;
    if (ptr) {
        (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    // 256 B of slack so 16-byte vector loads at the tail stay inside the allocation
    hipError_t e = hipMalloc(&ptr, bytes + 256);
    if (e != hipSuccess) {
        ptr = nullptr;
        return fail(WFA_E_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    cap = bytes;
    return WFA_OK;
}

void DevBuf::release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
}

static int use_device(wfa_ctx* c) {
    if (!c) return fail(WFA_E_INVALID, "null context");
    WFA_HIP_CHECK(hipSetDevice(c->device));
    return WFA_OK;
}

constexpr size_t kStageBytes = 32u << 20;   // per staging buffer
constexpr size_t kStageMin = 4u << 20;      // smaller copies go straight through hipMemcpyAsync

// the pinned staging ring of the context, created by its first large copy in either direction
static int ensure_stage(wfa_ctx* c) {
    if (c->stage[0]) return WFA_OK;
    for (int b = 0; b < 2; ++b) {
        WFA_HIP_CHECK(hipHostMalloc(&c->stage[b], kStageBytes, hipHostMallocDefault));
        WFA_HIP_CHECK(hipEventCreateWithFlags(&c->stage_ev[b], hipEventDisableTiming));
    }
    c->stage_bytes = kStageBytes;
    return WFA_OK;
}

// host -> device through the context's pinned double buffer (see wfa_ctx::stage; the ring itself: wfa_host.hpp); returns
// when the last chunk has landed
static int h2d_staged(wfa_ctx* c, void* dst, const void* src, size_t bytes) {
    if (int rc = ensure_stage(c)) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t err = hipSuccess;
    const int rc = host::staged_copy(
        dst, src, bytes, c->stage, kStageBytes,
        [&](void* d, const void* staged, size_t n, int b) {
            err = hipMemcpyAsync(d, staged, n, hipMemcpyHostToDevice, c->stream);
            if (err == hipSuccess) err = hipEventRecord(c->stage_ev[b], c->stream);
            return err == hipSuccess ? 0 : 1;
        },
        [&](int b) { return (err = hipEventSynchronize(c->stage_ev[b])) == hipSuccess ? 0 : 1; });
    if (rc) return fail(WFA_E_HIP, "staged upload failed: %s", hipGetErrorString(err));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));  // the staging buffers are free again for the next call
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (s > 0) c->last_h2d_GBps = (double)bytes / s / 1e9;
    return WFA_OK;
}

int h2d_copy(wfa_ctx* c, void* dst, const void* src, size_t bytes) {
    if (bytes >= kStageMin) return h2d_staged(c, dst, src, bytes);
    if (bytes) WFA_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    return WFA_OK;
}

int d2h_staged(wfa_ctx* c, void* dst, const void* src, size_t bytes, int (*queued)(void*), void* arg) {
    if (int rc = ensure_stage(c)) return rc;
    size_t prev_off = 0, prev_n = 0;
    int b = 0;
    for (size_t off = 0; off < bytes || prev_n; off += kStageBytes, b ^= 1) {
        const size_t n = off < bytes ? std::min(bytes - off, kStageBytes) : 0;
        if (n) {  // stage[b] is free: its last chunk was copied out one iteration ago
            WFA_HIP_CHECK(hipMemcpyAsync(c->stage[b], (const char*)src + off, n, hipMemcpyDeviceToHost, c->stream));
            WFA_HIP_CHECK(hipEventRecord(c->stage_ev[b], c->stream));
            if (off == 0 && queued)
                if (int rc = queued(arg)) return rc;
        }
        if (prev_n) {
            WFA_HIP_CHECK(hipEventSynchronize(c->stage_ev[b ^ 1]));
            host::parallel_memcpy((char*)dst + prev_off, c->stage[b ^ 1], prev_n);
        }
        prev_off = off;
        prev_n = n;
    }
    if (bytes == 0 && queued)
        if (int rc = queued(arg)) return rc;
    return WFA_OK;
}

static int h2d(wfa_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    int rc = b.ensure(bytes);
    if (rc) return rc;
    if (bytes >= kStageMin) return h2d_staged(c, b.ptr, src, bytes);
    if (bytes) WFA_HIP_CHECK(hipMemcpyAsync(b.ptr, src, bytes, hipMemcpyHostToDevice, c->stream));
    return WFA_OK;
}

static PoolView pool_view(wfa_ctx* c) {
    PoolView p;
    p.u16 = c->have_u16 ? c->pool_u16.as<uint16_t>() : nullptr;
    p.f32 = c->have_f32 ? c->pool_f32.as<float>() : nullptr;
    p.n = c->pool_n;
    return p;
}

// thr: the threshold column the kernels compare against (a hit pass: HitPass::thr)
static RecView rec_view(wfa_ctx* c, const double* thr) {
    RecView r;
    r.R = c->R;
    r.off = c->off.as<int64_t>();
    r.len = c->len.as<int32_t>();
    r.baseline = c->baseline.as<double>();
    r.baseline_rw = c->baseline.as<double>();
    r.pol = c->pol.as<int8_t>();
    r.thr = thr;
    r.ts = c->ts.as<int64_t>();
    r.dt = c->dt.as<int32_t>();
    r.board = c->board.as<int16_t>();
    r.chan = c->chan.as<int16_t>();
    r.rid = c->rid.as<int64_t>();
    r.bm_off = c->bm_off.as<int64_t>();
    return r;
}
static RecView rec_view(wfa_ctx* c) { return rec_view(c, c->thr.as<double>()); }  // the uploaded thresholds

// the context's own plan (wfa_set_sg_plan), null before the first one
static const SgPlanDev* ctx_plan(wfa_ctx* c) { return c->have_sg ? &c->sg : nullptr; }

static SgParams sg_params(const SgPlanDev* plan) {
    SgParams s{};
    if (!plan) return s;
    s.W = plan->W; s.P = plan->P; s.H = plan->H; s.stride = plan->stride;
    s.tab = plan->tab.as<double>();
    s.sym = plan->sym.as<uint8_t>();
    s.int_ok = plan->int_ok;
    s.itab = plan->itab.as<int32_t>();
    s.den = plan->den; s.den_edge = plan->den_edge;
    s.guard = plan->guard; s.guard_edge = plan->guard_edge;
    s.rden = plan->rden; s.rden_edge = plan->rden_edge;
    // |y| < 2^17 for uint16 samples (sum|c| < 2): float32 ulp <= 2^-7
    s.margin = (int32_t)((plan->den + 127) / 128 + 2);
    s.margin_edge = (int32_t)((plan->den_edge + 127) / 128 + 2);
    return s;
}

static int need_source(wfa_ctx* c, int source, const SgPlanDev* plan) {
    if (!c->have_records) return fail(WFA_E_STATE, "records not uploaded");
    switch (source) {
        case WFA_SRC_RAW:
            if (!c->have_u16) return fail(WFA_E_STATE, "wave_pool (uint16) not uploaded");
            return WFA_OK;
        case WFA_SRC_F32:
            if (!c->have_f32) return fail(WFA_E_STATE, "wave_pool_filtered (float32) not resident");
            return WFA_OK;
        case WFA_SRC_SG_FUSED:
            if (!c->have_u16) return fail(WFA_E_STATE, "wave_pool (uint16) not uploaded");
            if (!plan) return fail(WFA_E_STATE, "Savitzky-Golay plan not set");
            return WFA_OK;
        default:
            return fail(WFA_E_INVALID, "unknown wave source %d", source);
    }
}
static int need_source(wfa_ctx* c, int source) { return need_source(c, source, ctx_plan(c)); }

// padded shadow of the u16 pool (see wfa_ctx::layout): built once per upload, on the device
static int ensure_shadow(wfa_ctx* c) {
    if (c->shadow_valid) return WFA_OK;
    int rc;
    const UniformLayout& u = c->layout;
    const size_t shadow_samples = (size_t)c->R * u.S;
    if ((rc = c->shadow_pool.ensure(shadow_samples * sizeof(uint16_t) + 256))) return rc;
    if ((rc = c->shadow_off.ensure((size_t)c->R * sizeof(int64_t)))) return rc;
    LaunchTimer t(c);
    WFA_HIP_CHECK(hipMemsetAsync(c->shadow_pool.as<uint8_t>() + shadow_samples * sizeof(uint16_t), 0, 256, c->stream));
    WFA_HIP_CHECK(launch_pad_rows(c->stream, c->pool_u16.as<uint16_t>(), u.off0, u.L, u.S, c->R,
                                  c->shadow_pool.as<uint16_t>(), c->shadow_off.as<int64_t>()));
    if ((rc = t.end("k_pad_rows (once per upload)"))) return rc;
    c->shadow_valid = true;
    return WFA_OK;
}

// The pool, the records and the record geometry a pass over uniform records reads: in place, or (padded) through the
// shadow, in which record r starts at sample r * S.  The one place that reads the shadow buffers; what of it a kernel's
// parameter block takes, and in which convention, is the consumer's business.
struct LayoutView {
    PoolView pool;
    RecView rec;        // (padded: `off` is the shadow's offsets column)
    int32_t L, S;       // record length and stride; S == L in place
    int64_t off0;       // first sample of record 0 in `pool`
    int positive;
};

static int layout_view(wfa_ctx* c, const double* thr, bool padded, LayoutView* v) {
    const UniformLayout& u = c->layout;
    *v = LayoutView{pool_view(c), rec_view(c, thr), u.L, u.L, u.off0, u.positive ? 1 : 0};
    if (!padded) return WFA_OK;
    if (int rc = ensure_shadow(c)) return rc;
    v->pool.u16 = c->shadow_pool.as<uint16_t>();
    v->pool.n = c->R * (int64_t)u.S;
    v->rec.off = c->shadow_off.as<int64_t>();
    v->S = u.S;
    v->off0 = 0;
    return WFA_OK;
}

// uniform records of the row stage (RowParams::uni_S: 0 = records back to back)
static void row_layout(RowParams& rp, const LayoutView& v) {
    rp.uni_L = v.L; rp.uni_S = v.S == v.L ? 0 : v.S; rp.uni_positive = v.positive; rp.uni_off0 = v.off0;
}

// ---- row stage of the fused hit pass (both routes) ----------------------------------------------------------------
// Speculative launch: a pass usually finds about as many hits as the previous one like it (HitPass::hint).  When the row
// buffers already hold that many (+12 %, + 4096), the descriptor kernel and the row kernels are launched for that bound
// straight away and take the real count from the device; the host reads it once, after everything is queued, or not at all
// (enqueue_only: wfa_hits_wait does).  Without one (no hint, buffers too small, speculate off), or when the pass finds
// more, the host reads the count and launches the rows for exactly that many, into row buffers sized with the same head
// room so that the next pass can speculate.
static int64_t rows_bound(int64_t hits) { return hits + hits / 8 + 4096; }

// accept-or-redo of a speculative launch: its rows stand when the pass found no more hits than the launch covered and no
// span's events overflowed (flags: RunsParams::flags of the streaming route, 0 on the bitmap route)
static bool spec_rows_stand(int64_t total, int64_t bound, int flags) { return total <= bound && flags == 0; }

// What a route supplies:
//   desc(rp)  enqueues its descriptor kernel (k_runs_to_desc / k_hit_runs) for the row bound in rp;
//   count()   without a speculative launch: enqueues what leaves the exact row count in *d_total (nothing on the bitmap
//             route, whose per-record scan has done so already);
//   ctrl      streaming route: its control words ([1]: event-overflow flags) and `groups` its group sums, both reported
//             and cleared by the last kernel of a queued pass; null on the bitmap route.
// o->overflow (state kNone): a span's events overflowed, the caller takes the general route.
template <class Desc, class Count>
static int run_rows(wfa_ctx* c, const HitPass& p, const PoolView& pv, const RecView& rv, const SgParams& sg, RowParams rp,
                    const int64_t* d_total, unsigned long long* ctrl, unsigned long long* groups, Desc desc, Count count,
                    HitOutcome* o) {
    int rc;
    auto rows = [&](int64_t n_rows) -> int {
        int r2;
        if ((r2 = desc(rp))) return r2;
        {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_hit_rows_fast(c->stream, pv, rv, sg, rp, c->hit_desc.as<int4>(), n_rows,
                                               c->hit_out.as<uint8_t>()));
            if ((r2 = t.end("k_hit_rows_flat"))) return r2;
        }
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_hit_rows_literal(c->stream, WFA_SRC_SG_FUSED, pv, rv, sg, rp, c->hit_desc.as<int4>(), n_rows,
                                              true, c->hit_out.as<uint8_t>()));
        return t.end("k_hit_rows_literal");
    };
    auto finish = [&](int64_t total) {
        c->rows_index = 1;
        o->state = HitOutcome::kCompleted;
        o->n_hits = total;
        return WFA_OK;
    };
    const int64_t held = (int64_t)std::min(c->hit_out.cap / 60, c->hit_desc.cap / sizeof(int4));
    const int64_t bound = rows_bound(p.hint);
    const bool spec = p.hint >= 0 && held >= bound && p.speculate;
    if (spec) {
        rp.cap = bound;
        rp.n_dev = d_total;
        if (p.enqueue_only) {  // nobody waits here: the row count goes to the pinned words
            if (ctrl) {  // written there by the pass's last kernel, with the control words; it clears them and the group sums
                rp.pass_report = c->h_total;
                rp.pass_ctrl = ctrl;
                rp.pass_groups = groups;
                rp.pass_n_groups = c->run_dirty_groups;
            }
            if ((rc = rows(bound))) return rc;
            if (ctrl) c->run_dirty_groups = 0;  // (bound >= 4096: the literal kernel, and its clear, are queued)
            else WFA_HIP_CHECK(hipMemcpyAsync(c->h_total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            c->rows_index = 1;
            o->state = HitOutcome::kQueued;
            o->bound = bound;
            o->runs32 = ctrl != nullptr;
            return WFA_OK;
        }
        if ((rc = rows(bound))) return rc;
    } else if ((rc = count())) {
        return rc;
    }
    int64_t total = 0;
    unsigned long long ctl = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&total, d_total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    if (ctrl) WFA_HIP_CHECK(hipMemcpyAsync(&ctl, ctrl + 1, sizeof(ctl), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    const int flags = (int)(ctl & 0xffffffffull);
    if (flags) {  // a span outgrew the event buffer of its wave or its slot
        o->overflow = true;
        return WFA_OK;
    }
    if (spec && spec_rows_stand(total, bound, flags)) return finish(total);
    rp.cap = 0;
    rp.n_dev = nullptr;
    const int64_t want = rows_bound(total);
    if ((rc = c->hit_out.ensure((size_t)want * 60))) return rc;
    if ((rc = c->hit_desc.ensure((size_t)want * sizeof(int4)))) return rc;
    if ((rc = rows(total))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return finish(total);
}

// Uniform records (span mode), Savitzky-Golay source: streaming kernel with ordered run events (wfa_stream.hip), then the
// row stage: k_sg_runs32 -> k_runs_to_desc -> row kernels (plus a scan of the per-span hit counts when the host needs the
// row count first).
// o->state stays kNone: the layout / options are outside what that kernel covers, or a span outgrew its event buffer
// (o->overflow) -- the caller takes the general route (per-record mask kernel + bitmap).
static int run_hits_runs32(wfa_ctx* c, const HitPass& p, HitOutcome* o) {
    if (c->no_runs32 || c->opt.no_runs32) return WFA_OK;
    const SgParams sp0 = sg_params(p.plan);
    const UniformLayout& u = c->layout;
    const bool in_place = u.span && u.L % 32 == 0;
    const bool padded = !in_place && u.pad && u.S % 32 == 0 && !c->opt.no_pad;
    if (!in_place && !padded) return WFA_OK;
    if (!sg_runs32_supported(sp0, u.L, padded ? u.S : u.L, p.bl_start, p.bl_end, p.fused_bl)) return WFA_OK;
    int rc;
    LayoutView v;
    if ((rc = layout_view(c, p.thr, padded, &v))) return rc;
    SpanParams sp{};
    sp.off0 = v.off0; sp.L = v.L; sp.S = v.S; sp.positive = v.positive;
    const int64_t R = c->R;
    int32_t g_wstride = 0, g_nseg = 0, g_segw = 0;
    sg_runs32_geometry(sp.S, &sp.rs, &g_wstride, &g_nseg, &g_segw);
    if (c->opt.span_records > 0 && c->opt.span_records < sp.rs) sp.rs = c->opt.span_records;
    sp.n_spans = (R + sp.rs - 1) / sp.rs;
    const int64_t ns = sp.n_spans;
    const int64_t nb = scan_blocks_for(ns);
    if ((rc = c->run_span_off.ensure((size_t)ns * sizeof(int64_t)))) return rc;
    if ((rc = c->run_span_cnt.ensure((size_t)ns * sizeof(int32_t)))) return rc;
    if ((rc = c->run_span_row0.ensure((size_t)ns * sizeof(int64_t)))) return rc;
    if ((rc = c->run_scan_blocks.ensure((size_t)(nb + 1) * sizeof(int64_t)))) return rc;
    const int64_t n_groups = (ns + 63) / 64;
    // a new allocation of the group sums or the control words may hold anything: dirty over its whole size
    const bool new_ctrl = c->run_ctrl.cap < 256 + sizeof(RunsCold);
    const bool new_groups = c->run_groups.cap < (size_t)n_groups * sizeof(unsigned long long);
    if ((rc = c->run_groups.ensure((size_t)n_groups * sizeof(unsigned long long)))) return rc;
    if ((rc = c->run_ctrl.ensure(256 + sizeof(RunsCold)))) return rc;
    if (new_ctrl) c->run_cold_valid = false;
    if (new_ctrl || new_groups) c->run_dirty_groups = (int64_t)(c->run_groups.cap / sizeof(unsigned long long));

    RowParams rp{p.le, p.re, p.max_len, sp0.W / 2};
    row_layout(rp, v);
    int64_t* d_total = c->run_scan_blocks.as<int64_t>() + nb;
    auto* ctrl = c->run_ctrl.as<unsigned long long>();  // [0] event cursor, [1] flags, [2] hits listed for the literal kernel
    constexpr int kLitCap = 65536;
    if ((rc = c->run_lit.ensure((size_t)kLitCap * sizeof(int32_t)))) return rc;
    rp.lit_cnt = reinterpret_cast<uint32_t*>(ctrl + 2);
    rp.lit_list = c->run_lit.as<int32_t>();
    rp.lit_cap = kLitCap;

    // every span owns a fixed slot of the event buffer (8 KiB: 160 MB per 10^9 samples, only the lines that hold events
    // are ever touched)
    const int64_t ev_want = ns * sg_runs32_event_slot();
    if ((int64_t)(c->run_ev.cap / sizeof(uint32_t)) < ev_want)
        if ((rc = c->run_ev.ensure((size_t)ev_want * sizeof(uint32_t)))) return rc;
    RunsParams rn{};
    rn.ev = c->run_ev.as<uint32_t>();
    rn.ev_cap = (int64_t)(c->run_ev.cap / sizeof(uint32_t));
    rn.cursor = ctrl;
    rn.flags = reinterpret_cast<int32_t*>(ctrl + 1);
    rn.span_off = c->run_span_off.as<int64_t>();
    rn.span_cnt = c->run_span_cnt.as<int32_t>();
    rn.group_sum = c->run_groups.as<unsigned long long>();
    rn.lit_cnt = rp.lit_cnt;
    // control words and group sums are zero between passes: a pass that finds them dirty clears the whole recorded extent
    if (c->run_dirty_groups > 0) {
        WFA_HIP_CHECK(hipMemsetAsync(ctrl, 0, 16, c->stream));
        WFA_HIP_CHECK(hipMemsetAsync(rn.group_sum, 0, (size_t)c->run_dirty_groups * sizeof(unsigned long long), c->stream));
        c->run_dirty_groups = 0;
    }
    RunsArgs ra{};
    ra.pool = v.pool.u16; ra.thr = v.rec.thr; ra.baseline = v.rec.baseline_rw; ra.R = R;
    ra.itab = sp0.itab; ra.den = sp0.den; ra.margin = sp0.margin;
    ra.den_edge = sp0.den_edge; ra.margin_edge = sp0.margin_edge;
    // sg_plan.py: guard = 8 eps den^2 2^24 + 1 with eps = bound on |scipy's float64 chain - exact rational|; here in
    // numerator units with a factor 4 of head room (and never below 1e-6)
    ra.delta = std::max(4.0 * (double)sp0.guard / (8.0 * (double)sp0.den * 16777216.0), 1e-6);
    ra.W = sp0.W; ra.L = sp.L; ra.S = sp.S; ra.positive = sp.positive; ra.rs = sp.rs;
    ra.wstride = g_wstride; ra.nseg = g_nseg; ra.segw = g_segw;
    ra.dep = (!c->opt.no_deposit && sg_runs32_deposit(sp.L, sp.S, sp0.W, sp.rs, g_wstride)) ? 1 : 0;
    ra.off0 = sp.off0; ra.n_spans = ns;
    ra.ev = rn.ev; ra.ev_cap = rn.ev_cap; ra.cursor = rn.cursor; ra.span_off = rn.span_off; ra.span_cnt = rn.span_cnt;
    ra.flags = rn.flags;
    ra.group_sum = rn.group_sum;
    ra.cold = reinterpret_cast<const RunsCold*>(ctrl + 32);  // 256 bytes behind the atomically updated words
    {
        // what the float64 reference paths read: a device copy next to the control words, refreshed when it changes, from
        // the pass's pinned slot; the slot is rewritten (an earlier copy from it may be in flight: wait) only when it differs
        RunsCold cold{v.pool, sp0};
        if (!c->run_cold_valid || memcmp(&cold, &c->run_cold_host, sizeof(cold)) != 0) {
            if (memcmp(p.cold_pin, &cold, sizeof(cold)) != 0) {
                WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
                memcpy(p.cold_pin, &cold, sizeof(cold));
            }
            WFA_HIP_CHECK(hipMemcpyAsync(ctrl + 32, p.cold_pin, sizeof(cold), hipMemcpyHostToDevice, c->stream));
            c->run_cold_host = cold;
            c->run_cold_valid = true;
        }
    }
    c->run_dirty_groups = n_groups;  // what the streaming kernel is about to write
    {
        LaunchTimer t(c, true);
        WFA_HIP_CHECK(launch_sg_runs32(c->stream, p.fused_bl, ra));
        if ((rc = t.end(p.fused_bl ? "k_sg_runs32<baseline>" : "k_sg_runs32"))) return rc;
    }
    auto desc = [&](const RowParams& r) -> int {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_runs_to_desc(c->stream, rn, ns, sp.rs, d_total, r.cap, c->hit_desc.as<int4>()));
        return t.end("k_runs_to_desc");
    };
    auto count = [&]() -> int {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_scan(c->stream, rn.span_cnt, ns, c->run_scan_blocks.as<int64_t>(),
                                  c->run_span_row0.as<int64_t>()));
        return t.end("k_scan(span hit counts)");
    };
    return run_rows(c, p, v.pool, v.rec, sp0, rp, d_total, ctrl, rn.group_sum, desc, count, o);
}

// One hit pass over the resident records as `p` describes it; *o says what it did.  A pass that starts ends the queued
// one and voids the rows of the last one; what the context remembers of this one (row count, hint, pending record) is
// the caller's to store.  p.enqueue_only: when the pass can take the speculative row launch, queue it and return without
// waiting for the row count (wfa_hits_wait delivers it); otherwise the pass runs to completion as usual.
static int run_hits(wfa_ctx* c, HitPass p, HitOutcome* o) {
    *o = HitOutcome{};
    int rc;
    if ((rc = need_source(c, p.source, p.plan))) return rc;
    c->pending = wfa_ctx::kPendNone;
    if (p.le < 0) p.le = 0;  // hit_finder.py:124-125
    if (p.re < 0) p.re = 0;
    if (p.max_len <= 0) p.max_len = c->max_len;
    if (p.max_len < c->max_len)
        return fail(WFA_E_INVALID, "max_len (%d) < longest uploaded record (%d)", p.max_len, c->max_len);
    if (p.fused_bl && p.bl_start < 0) return fail(WFA_E_INVALID, "baseline window start must be >= 0");
    if (p.fused_bl) {
        const host::BaselineWindow w = host::baseline_window(p.bl_start, p.bl_end, c->max_len);
        p.bl_start = w.start; p.bl_end = w.end;
    }
    const int source = p.source, bl_start = p.bl_start, bl_end = p.bl_end;
    const bool fused_bl = p.fused_bl;
    c->n_hits = -1;
    c->rows_index = 0;
    if (c->R == 0) {
        o->state = HitOutcome::kCompleted;
        o->n_hits = 0;
        return WFA_OK;
    }

    const int64_t R = c->R;
    if ((rc = c->rec_tmp_start.ensure(R * sizeof(int64_t)))) return rc;
    if ((rc = c->rec_nhits.ensure(R * sizeof(int32_t)))) return rc;
    if ((rc = c->rec_out_start.ensure(R * sizeof(int64_t)))) return rc;
    const int64_t nb = scan_blocks_for(R);
    if ((rc = c->scan_blocks.ensure((nb + 1) * sizeof(int64_t)))) return rc;
    if ((rc = c->cursor.ensure(sizeof(unsigned long long)))) return rc;

    const SgParams sp0 = sg_params(p.plan);
    if (source == WFA_SRC_SG_FUSED && sg_mask_supported(sp0) && !c->opt.no_fast) {
        if ((rc = run_hits_runs32(c, p, o))) return rc;
        if (o->state != HitOutcome::kNone) return WFA_OK;
        if (o->overflow) c->no_runs32 = true;  // the general route for this upload
        // A: mask + run counts  ->  scan  ->  B1: run descriptors  ->  B2: rows (final order, no gather)
        if (c->bitmap.cap < (size_t)c->bitmap_bytes) c->bitmap_clean = false;
        if ((rc = c->bitmap.ensure((size_t)c->bitmap_bytes))) return rc;
        if (!c->bitmap_clean) {  // bytes between a record's last mask byte and its next word stay zero
            WFA_HIP_CHECK(hipMemsetAsync(c->bitmap.ptr, 0, (size_t)c->bitmap_bytes, c->stream));
            c->bitmap_clean = true;
        }
        MaskParams mp{};
        mp.bl_start = bl_start; mp.bl_end = fused_bl ? bl_end : bl_start;
        mp.bitmap = c->bitmap.as<uint8_t>();
        mp.rec_nhits = c->rec_nhits.as<int32_t>();
        // views the kernels of this pass read: the uploaded layout, or the padded shadow of it
        const UniformLayout& u = c->layout;
        const bool padded = u.pad && sg_mask_span16_padded_supported(sp0, u.L) && !c->opt.no_pad && !c->opt.no_span;
        LayoutView v;
        if ((rc = layout_view(c, p.thr, padded, &v))) return rc;
        {
            LaunchTimer t(c, true);
            if (padded || (u.span && u.L >= sp0.W && !c->opt.no_span && sg_mask_span16_supported(sp0, u.L))) {
                SpanParams sp{};
                sp.off0 = v.off0; sp.L = v.L; sp.positive = v.positive;
                if (padded) sp.S = v.S;  // (in place: 0)
                sp.rs = 64;
                sp.n_spans = (R + sp.rs - 1) / sp.rs;
                sp.bm_off0 = 0;
                sp.bm_stride = ((int64_t)sp.L + 7 + 63) / 64 * 8 + 8;
                WFA_HIP_CHECK(launch_sg_mask_span16(c->stream, fused_bl, v.pool, v.rec, sp0, mp, sp));
                if ((rc = t.end(fused_bl ? "k_sg_mask_span16<baseline>" : "k_sg_mask_span16"))) return rc;
            } else {
                WFA_HIP_CHECK(launch_sg_mask(c->stream, fused_bl, c->max_len, v.pool, v.rec, sp0, mp));
                if ((rc = t.end(fused_bl ? "k_sg_mask<baseline>" : "k_sg_mask"))) return rc;
            }
        }
        {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_scan(c->stream, c->rec_nhits.as<int32_t>(), R, c->scan_blocks.as<int64_t>(),
                                      c->rec_out_start.as<int64_t>()));
            if ((rc = t.end("k_scan(hit counts)"))) return rc;
        }
        RowParams rp{p.le, p.re, p.max_len, sp0.W / 2};
        if (padded || u.span) row_layout(rp, v);
        {
            // mask bytes of one block's records (+16 for the aligned start), rounded up to 1 KiB
            const int64_t per_rec = ((int64_t)c->max_len + 7 + 63) / 64 * 8 + 8;
            const int64_t need = (per_rec * hit_runs_block() + 16 + 1023) / 1024 * 1024;
            rp.stage_bytes = need <= 48 * 1024 ? (int32_t)need : 48 * 1024;
        }
        auto desc = [&](const RowParams& r) -> int {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_hit_runs(c->stream, v.rec, c->bitmap.as<uint8_t>(), c->rec_nhits.as<int32_t>(),
                                          c->rec_out_start.as<int64_t>(), c->hit_desc.as<int4>(), r));
            return t.end("k_hit_runs");
        };
        // (no event buffers on this route: queued or completed)
        return run_rows(c, p, v.pool, v.rec, sp0, rp, c->scan_blocks.as<int64_t>() + nb, nullptr, nullptr, desc,
                        [] { return WFA_OK; }, o);
    }

    HitParams hp{};
    hp.le = p.le; hp.re = p.re; hp.max_len = p.max_len;
    hp.bl_start = bl_start; hp.bl_end = bl_end;
    hp.bm_words = (c->max_len + 7 + 63) / 64 + 9;  // bits are indexed from the 16-byte aligned base
    hp.chunk_rows = 256;
    hp.use_fast = c->opt.no_fast ? 0 : 1;
    const int64_t waves = hits_waves(R);
    int64_t want_rows = waves * hp.chunk_rows + c->pool_n / 256 + 4096;
    if (c->hit_tmp_rows < want_rows) {
        if ((rc = c->hit_tmp.ensure((size_t)want_rows * 60))) return rc;
        c->hit_tmp_rows = want_rows;
    }

    const PoolView pv = pool_view(c);
    const RecView rv = rec_view(c, p.thr);
    for (int attempt = 0; attempt < 2; ++attempt) {
        hp.tmp = c->hit_tmp.as<uint8_t>();
        hp.tmp_rows = c->hit_tmp_rows;
        hp.cursor = c->cursor.as<unsigned long long>();
        hp.rec_tmp_start = c->rec_tmp_start.as<int64_t>();
        hp.rec_nhits = c->rec_nhits.as<int32_t>();
        WFA_HIP_CHECK(hipMemsetAsync(c->cursor.ptr, 0, sizeof(unsigned long long), c->stream));
        {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_hits(c->stream, source, fused_bl, pv, rv, sp0, hp));
            const char* name = source == WFA_SRC_SG_FUSED
                                   ? (fused_bl ? "k_hits<sg_fused,baseline>" : "k_hits<sg_fused>")
                                   : (source == WFA_SRC_F32 ? "k_hits<f32>" : (fused_bl ? "k_hits<raw,baseline>" : "k_hits<raw>"));
            if ((rc = t.end(name))) return rc;
        }
        unsigned long long used = 0;
        WFA_HIP_CHECK(hipMemcpyAsync(&used, c->cursor.ptr, sizeof(used), hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        if ((int64_t)used <= c->hit_tmp_rows) break;
        if (attempt == 1) return fail(WFA_E_NOMEM, "hit scratch overflow after regrow");
        // chunk placement is deterministic for a fixed grid: `used` rows are enough
        const int64_t rows = (int64_t)used + 1024;
        if ((rc = c->hit_tmp.ensure((size_t)rows * 60))) return rc;
        c->hit_tmp_rows = rows;
    }

    {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_scan(c->stream, c->rec_nhits.as<int32_t>(), R, c->scan_blocks.as<int64_t>(),
                                  c->rec_out_start.as<int64_t>()));
        if ((rc = t.end("k_scan(hit counts)"))) return rc;
    }
    int64_t total = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&total, c->scan_blocks.as<int64_t>() + nb, sizeof(int64_t),
                                 hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = c->hit_out.ensure((size_t)total * 60))) return rc;
    {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_hits_gather(c->stream, c->hit_tmp.as<uint8_t>(), c->rec_tmp_start.as<int64_t>(),
                                         c->rec_nhits.as<int32_t>(), c->rec_out_start.as<int64_t>(), R,
                                         c->hit_out.as<uint8_t>()));
        if ((rc = t.end("k_hits_gather"))) return rc;
    }
    c->rows_index = 2;
    o->state = HitOutcome::kCompleted;
    o->n_hits = total;
    return WFA_OK;
}

// The single pass of the public entry points: described from the context's own plan, thresholds, hint and options, what
// it did stored back.  The hint follows the passes with a row stage (rows_index 1).  n_hits: null if enqueue_only.
static int ctx_pass(wfa_ctx* c, int source, bool fused_bl, int32_t bl_start, int32_t bl_end, int32_t le, int32_t re,
                    int32_t max_len, int64_t* n_hits, bool enqueue_only) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!n_hits && !enqueue_only) return fail(WFA_E_INVALID, "n_hits is null");
    HitPass p;
    p.source = source; p.plan = ctx_plan(c); p.thr = c->thr.as<double>();
    p.fused_bl = fused_bl; p.bl_start = bl_start; p.bl_end = bl_end; p.le = le; p.re = re; p.max_len = max_len;
    p.hint = c->last_hits; p.speculate = !c->opt.no_speculate; p.enqueue_only = enqueue_only; p.cold_pin = c->h_cold;
    HitOutcome o;
    if ((rc = run_hits(c, p, &o))) return rc;
    if (o.state == HitOutcome::kQueued) {
        c->pending = wfa_ctx::kPendPass;
        c->pend = {p, o};
        return WFA_OK;
    }
    c->n_hits = o.n_hits;
    if (c->rows_index == 1) c->last_hits = o.n_hits;
    if (n_hits) *n_hits = o.n_hits;
    return WFA_OK;
}

// A queued single pass has ended (the stream is idle): its row count and overflow flags from the pinned words, what they
// mean for the next passes, and whether its speculative rows stand (otherwise the caller redoes the pass the exact way).
static bool pass_settle(wfa_ctx* c, int64_t bound, bool runs32, int64_t* total) {
    *total = *c->h_total;
    const int flags = runs32 ? (int)(c->h_total[2] & 0xffffffffll) : 0;  // event buffers overflowed
    if (flags) c->no_runs32 = true;  // a span outgrew its LDS buffer or its slot: the general route from now on
    c->last_hits = *total;
    return spec_rows_stand(*total, bound, flags);
}

}  // namespace wfa

using namespace wfa;

static int groups_wait(wfa_ctx* c, int64_t* n_hits);  // a queued grouped pass (wfa_hits_enqueue_groups, below)

// ---- records as packed rows, unpacked on the device --------------------------------------------------------------------
// (reference row layout: processing/dtypes.py:80-100, 102 bytes, numpy packs without alignment.)  The column route above
// makes the caller extract ten columns on the host -- for 1.25e6 records that is 0.6 s of numpy, 0.47 s of it comparing
// the 32-byte `polarity` strings -- before 1 ms of GPU work.  Here the rows go through the pinned staging ring as they are
// (128 MB: 3 ms) and one kernel writes the columns, validates them and finds what the host loop above finds.
struct PackedFields {  // byte offsets inside a row; -1 = field absent (default used)
    int32_t off, len, baseline, polarity, ts, dt, board, chan, rid;
    int32_t polarity_chars;  // width of the UCS-4 polarity field in characters (>= 8)
    int32_t row_bytes;
};
struct UnpackResult {  // one per upload, device -> host
    unsigned long long first_bad[4];  // first record with: negative offset, negative length, out of pool, too long
    int max_len;
    int nonuniform;       // some record breaks (len == len0, off == off0 + r len0, polarity class == class 0)
    int rid_not_increasing;
    int pad;
};

template <typename T>
__device__ __forceinline__ T load_unaligned(const uint8_t* p) {
    T v;
    uint8_t b[sizeof(T)];
#pragma unroll
    for (size_t i = 0; i < sizeof(T); ++i) b[i] = p[i];
    __builtin_memcpy(&v, b, sizeof(T));
    return v;
}

__device__ __forceinline__ bool ucs4_equals(const uint8_t* p, int chars, const char* word) {  // `word` has 8 letters
    bool eq = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) eq = eq && load_unaligned<uint32_t>(p + 4 * i) == (uint32_t)(unsigned char)word[i];
    if (chars > 8) eq = eq && load_unaligned<uint32_t>(p + 32) == 0u;
    return eq;
}

__global__ __launch_bounds__(256) void k_unpack_records(const uint8_t* __restrict__ rows, int64_t R, PackedFields f,
                                                         int64_t pool_n, double thr_scalar, const double* __restrict__ thr_in,
                                                         const int8_t* __restrict__ pol_in, RecView out_cols,
                                                         int8_t* __restrict__ out_pol, double* __restrict__ out_thr,
                                                         int64_t* __restrict__ out_off, int32_t* __restrict__ out_len,
                                                         int64_t* __restrict__ out_ts, int32_t* __restrict__ out_dt,
                                                         int16_t* __restrict__ out_board, int16_t* __restrict__ out_chan,
                                                         int64_t* __restrict__ out_rid, int32_t* __restrict__ bm_bytes,
                                                         UnpackResult* __restrict__ res) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const uint8_t* row = rows + r * f.row_bytes;
    const int64_t off = load_unaligned<int64_t>(row + f.off);
    const int32_t len = load_unaligned<int32_t>(row + f.len);
    auto pol_of = [&](const uint8_t* rw) -> int8_t {
        if (f.polarity < 0) return WFA_POL_UNKNOWN;
        if (ucs4_equals(rw + f.polarity, f.polarity_chars, "negative")) return WFA_POL_NEGATIVE;
        if (ucs4_equals(rw + f.polarity, f.polarity_chars, "positive")) return WFA_POL_POSITIVE;
        return WFA_POL_UNKNOWN;
    };
    const int8_t pol = pol_in ? pol_in[r] : pol_of(row);
    const int64_t rid = load_unaligned<int64_t>(row + f.rid);
    out_off[r] = off;
    out_len[r] = len;
    out_cols.baseline_rw[r] = load_unaligned<double>(row + f.baseline);
    out_pol[r] = pol;
    out_thr[r] = thr_in ? thr_in[r] : thr_scalar;
    out_ts[r] = load_unaligned<int64_t>(row + f.ts);
    out_dt[r] = f.dt >= 0 ? load_unaligned<int32_t>(row + f.dt) : 1;
    out_board[r] = f.board >= 0 ? load_unaligned<int16_t>(row + f.board) : (int16_t)0;
    out_chan[r] = f.chan >= 0 ? load_unaligned<int16_t>(row + f.chan) : (int16_t)0;
    out_rid[r] = rid;
    bm_bytes[r] = (int32_t)(((int64_t)(len > 0 ? len : 0) + 7 + 63) / 64 * 8 + 8);
    // the checks of the column route, first offender per kind (the host reports the earliest one)
    if (off < 0) atomicMin(&res->first_bad[0], (unsigned long long)r);
    if (len < 0) atomicMin(&res->first_bad[1], (unsigned long long)r);
    if (off >= 0 && len >= 0 && off + (int64_t)len > pool_n) atomicMin(&res->first_bad[2], (unsigned long long)r);
    if (len > WFA_MAX_RECORD_SAMPLES) atomicMin(&res->first_bad[3], (unsigned long long)r);
    if (len > 0) atomicMax(&res->max_len, len);
    // uniform layout (span mode / padded shadow): against record 0, read again by every thread (one cached line)
    const int64_t off0 = load_unaligned<int64_t>(rows + f.off);
    const int32_t len0 = load_unaligned<int32_t>(rows + f.len);
    const int8_t pol0 = pol_in ? pol_in[0] : pol_of(rows);
    if (len != len0 || off != off0 + r * (int64_t)len0 || (pol == WFA_POL_POSITIVE) != (pol0 == WFA_POL_POSITIVE))
        atomicOr(&res->nonuniform, 1);
    if (r > 0 && rid <= load_unaligned<int64_t>(row - f.row_bytes + f.rid)) atomicOr(&res->rid_not_increasing, 1);
}

// ---- dense rows (st_waveforms / filtered_waveforms), unpacked on the device -------------------------------------------
// (reference: cpu/_wave_source.py load_wave_input hands the structured array to the dense branches, which read
// data["wave"] -- a strided view of rows of 76 + 2 L bytes -- row by row.)  The rows go through the staging ring as they
// are; a lane owns 16 bytes of the row-major pool and collects them from the rows of the batch (host::dense_unpack_lane,
// wfa_host.hpp: the same function runs over exactly-sized buffers in host_check).  W = bytes per load, chosen on the host
// from the alignment of (wave_offset, row_bytes).
template <int ES, int W, bool SIGNED>
__global__ __launch_bounds__(256) void k_dense_unpack(const uint8_t* __restrict__ rows, uint8_t* __restrict__ pool,
                                                       host::DenseBatch b, uint64_t chunk0, uint32_t n_chunks,
                                                       unsigned long long* __restrict__ first_negative) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_chunks) return;
    const int64_t neg = host::dense_unpack_lane<ES, W, SIGNED>(rows, pool, b, chunk0 + g);
    if constexpr (SIGNED) {
        // (the plain read only spares the atomic once an earlier row is known: the word never grows)
        if (neg >= 0 && (unsigned long long)neg < *(volatile unsigned long long*)first_negative)
            atomicMin(first_negative, (unsigned long long)neg);
    }
}

template <int ES, bool SIGNED>
static int launch_dense_unpack(int load_bytes, hipStream_t stream, const uint8_t* rows, uint8_t* pool,
                               const host::DenseBatch& b, unsigned long long* first_negative) {
    const uint64_t chunk0 = host::dense_first_chunk(b, ES);
    const uint64_t chunks = host::dense_chunk_count(b, ES);
    if (chunks == 0) return WFA_OK;
    if (chunks > 0xffffffffull) return fail(WFA_E_LIMIT, "dense batch too large");
    const dim3 grid((unsigned)((chunks + 255) / 256)), block(256);
    const uint32_t n = (uint32_t)chunks;
    switch (load_bytes) {
        case 2:
            if constexpr (ES == 2) {
                hipLaunchKernelGGL((k_dense_unpack<ES, 2, SIGNED>), grid, block, 0, stream, rows, pool, b, chunk0, n, first_negative);
                break;
            }
            return fail(WFA_E_INVALID, "load width below the element size");
        case 4: hipLaunchKernelGGL((k_dense_unpack<ES, 4, SIGNED>), grid, block, 0, stream, rows, pool, b, chunk0, n, first_negative); break;
        case 8: hipLaunchKernelGGL((k_dense_unpack<ES, 8, SIGNED>), grid, block, 0, stream, rows, pool, b, chunk0, n, first_negative); break;
        case 16: hipLaunchKernelGGL((k_dense_unpack<ES, 16, SIGNED>), grid, block, 0, stream, rows, pool, b, chunk0, n, first_negative); break;
        default: return fail(WFA_E_INVALID, "bad load width %d", load_bytes);
    }
    WFA_HIP_CHECK(hipGetLastError());
    return WFA_OK;
}

// the second stream and the three events of wfa_upload_dense_rows (see wfa_ctx::dense_stream)
static int ensure_dense_stream(wfa_ctx* c) {
    if (!c->dense_stream) WFA_HIP_CHECK(hipStreamCreateWithFlags(&c->dense_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : c->dense_ev)
        if (!e) WFA_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return WFA_OK;
}


extern "C" {

int wfa_abi_version(void) { return WFA_ABI_VERSION; }

int wfa_device_count(int* count) {
    if (!count) return fail(WFA_E_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(WFA_E_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *count = n;
    return WFA_OK;
}

int wfa_last_error(char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return WFA_E_INVALID;
    snprintf(buf, buf_len, "%s", g_last_error.c_str());
    return WFA_OK;
}

int wfa_ctx_create(int device_id, wfa_ctx** out) {
    if (!out) return fail(WFA_E_INVALID, "out is null");
    *out = nullptr;
    int n = 0;
    WFA_HIP_CHECK(hipGetDeviceCount(&n));
    if (device_id < 0 || device_id >= n)
        return fail(WFA_E_INVALID, "device %d out of range (have %d)", device_id, n);
    WFA_HIP_CHECK(hipSetDevice(device_id));
    wfa_ctx* c = new (std::nothrow) wfa_ctx();
    if (!c) return fail(WFA_E_NOMEM, "out of host memory");
    c->device = device_id;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&c->ev0);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->h_total), 4 * sizeof(int64_t) + sizeof(wfa::RunsCold), hipHostMallocDefault);
    if (e == hipSuccess) c->h_cold = reinterpret_cast<wfa::RunsCold*>(c->h_total + 4);
    if (e == hipSuccess) memset(c->h_cold, 0, sizeof(wfa::RunsCold));  // (a pass compares the slot with the block it needs)
    if (e == hipSuccess) e = hipEventCreate(&c->ev1);
    if (e != hipSuccess) {
        wfa_ctx_destroy(c);
        return fail(WFA_E_HIP, "context setup failed: %s", hipGetErrorString(e));
    }
    *out = c;
    return WFA_OK;
}

void wfa_ctx_destroy(wfa_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->comm) (void)wfa_rccl_destroy(c);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->h_total) (void)hipHostFree(c->h_total);
    if (c->h_grp) (void)hipHostFree(c->h_grp);
    for (int b = 0; b < 2; ++b) {
        if (c->stage[b]) (void)hipHostFree(c->stage[b]);
        if (c->stage_ev[b]) (void)hipEventDestroy(c->stage_ev[b]);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->dense_stream) (void)hipStreamSynchronize(c->dense_stream);
    for (hipEvent_t e : c->dense_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->dense_stream) (void)hipStreamDestroy(c->dense_stream);
    (void)profile_flush(c);
    for (hipEvent_t e : c->prof_free) (void)hipEventDestroy(e);
    c->prof_free.clear();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;  // every DevBuf frees its memory
}

int wfa_scratch_bytes(wfa_ctx* c, int64_t* bytes) {
    if (!c || !bytes) return fail(WFA_E_INVALID, "null argument");
    int64_t held = 0;
    for (DevBuf* b : c->scratch) held += (int64_t)b->cap;
    *bytes = held;
    return WFA_OK;
}

int wfa_release_scratch(wfa_ctx* c, int64_t* freed_bytes) {
    if (!c) return fail(WFA_E_INVALID, "null context");
    WFA_HIP_CHECK(hipSetDevice(c->device));
    if (c->stream) WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    // what a later call rebuilds by itself.  Kept: the resident pools, the records columns, the filter plan, the rows of the
    // last passes (hit_out / hit_desc / peak_out / out_rows / gathered: *_fill and the resident hit-table stages read them),
    // the CSV sample arena (source of wfa_csv_arena_gather), the carry and the last rows of an open event, merge,
    // merged-event or df_events stream (state between pushes, freed by the stream's _end), the pinned staging ring and the
    // small control blocks.  The
    // samples of the last wfa_csv_decode_fill live in a scratch slot: they go, and wfa_pool_gather(src_pool = NULL) refuses
    // until the next decode.
    int64_t freed = 0;
    for (DevBuf* b : c->scratch) { freed += (int64_t)b->cap; b->release(); }  // (a count pass without its fill is void after this)
    c->ht_n = -1;
    c->ht_perm = nullptr;
    c->n_chain = -1;
    c->csv_rows = -1;
    c->csv_samples = -1;
    c->csv_filled = false;
    pass_caches_dropped(c);
    c->hit_tmp_rows = 0;
    if (freed_bytes) *freed_bytes = freed;
    return WFA_OK;
}

int wfa_set_option(wfa_ctx* c, const char* name, int value) {
    if (!c || !name) return fail(WFA_E_INVALID, "null argument");
    const std::string n(name);
    const bool v = value != 0;
    if (n == "no_fast") c->opt.no_fast = v;
    else if (n == "no_span") c->opt.no_span = v;
    else if (n == "no_pad") c->opt.no_pad = v;
    else if (n == "no_runs32") c->opt.no_runs32 = v;
    else if (n == "no_speculate") c->opt.no_speculate = v;
    else if (n == "no_peak_slots") c->opt.no_peak_slots = v;
    else if (n == "no_peak_hot") c->opt.no_peak_hot = v;
    else if (n == "no_deposit") c->opt.no_deposit = v;
    else if (n == "span_records") c->opt.span_records = value;  // streaming kernel: records per span (0 = chosen by the library)
    else return fail(WFA_E_INVALID, "unknown option '%s'", name);
    return WFA_OK;
}

int wfa_last_h2d_rate(wfa_ctx* c, double* gb_per_s) {
    if (!c || !gb_per_s) return fail(WFA_E_INVALID, "null argument");
    *gb_per_s = c->last_h2d_GBps;
    return WFA_OK;
}

int wfa_sync(wfa_ctx* c) {
    int rc = use_device(c);
    if (rc) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_upload_pool_u16(wfa_ctx* c, const uint16_t* pool, int64_t n) {
    int rc = use_device(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !pool)) return fail(WFA_E_INVALID, "bad wave_pool argument");
    if ((rc = h2d(c, c->pool_u16, pool, (size_t)n * sizeof(uint16_t)))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    pool_replaced(c, n, true);
    return WFA_OK;
}

int wfa_upload_pool_f32(wfa_ctx* c, const float* pool, int64_t n) {
    int rc = use_device(c);
    if (rc) return rc;
    if (n < 0 || (n > 0 && !pool)) return fail(WFA_E_INVALID, "bad wave_pool_filtered argument");
    if (c->have_u16 && n != c->pool_n) c->have_u16 = false;  // a different run: the resident wave_pool is stale
    if ((rc = h2d(c, c->pool_f32, pool, (size_t)n * sizeof(float)))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    pool_replaced(c, n, false);
    return WFA_OK;
}

int wfa_upload_dense_rows(wfa_ctx* c, const void* rows, int64_t n_rows, int64_t row_bytes, int32_t wave_offset,
                          int32_t wave_length, int elem, int64_t batch_bytes, int64_t* first_negative_row) {
    int rc = use_device(c);
    if (rc) return rc;
    if (first_negative_row) *first_negative_row = -1;
    if (elem != WFA_DENSE_I16 && elem != WFA_DENSE_U16 && elem != WFA_DENSE_F32)
        return fail(WFA_E_INVALID, "unknown dense element type %d", elem);
    const int es = elem == WFA_DENSE_F32 ? 4 : 2;
    const bool u16 = es == 2;
    if (n_rows < 0 || row_bytes < 0 || wave_offset < 0 || wave_length < 0) return fail(WFA_E_INVALID, "negative size");
    if (wave_offset % es != 0 || row_bytes % es != 0)
        return fail(WFA_E_INVALID, "wave_offset %d and row_bytes %lld must be multiples of the element size %d", wave_offset,
                    (long long)row_bytes, es);
    if ((int64_t)wave_offset + (int64_t)wave_length * es > row_bytes)
        return fail(WFA_E_INVALID, "wave of %d elements at byte %d does not fit a %lld-byte row", wave_length, wave_offset,
                    (long long)row_bytes);
    const int64_t n = n_rows * (int64_t)wave_length;
    if (n > 0 && !rows) return fail(WFA_E_INVALID, "rows is null");
    DevBuf& pool = u16 ? c->pool_u16 : c->pool_f32;
    int64_t rows_per_batch = 0;
    if (n > 0) {
        rows_per_batch = host::dense_rows_per_batch(n_rows, row_bytes, batch_bytes);
        if ((uint64_t)rows_per_batch * (uint64_t)row_bytes >= (1ull << 31))
            return fail(WFA_E_LIMIT, "row of %lld bytes too long", (long long)row_bytes);
    }
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));  // nothing reads the pool that is about to change
    if ((rc = pool.ensure((size_t)n * es))) return rc;
    // from here on a failure leaves the context without this pool (and, for a wave_pool, without records)
    if (u16) {
        c->have_u16 = c->have_f32 = c->filter_keep = false;
        records_dropped(c);
    } else {
        if (c->have_u16 && n != c->pool_n) c->have_u16 = false;  // a different run: the resident wave_pool is stale
        c->have_f32 = false;
    }
    if (n > 0) {
        const size_t buf_bytes = (size_t)rows_per_batch * (size_t)row_bytes;
        if ((rc = ensure_dense_stream(c)) || (rc = c->dense_rows[0].ensure(buf_bytes)) ||
            (rc = c->dense_rows[1].ensure(n_rows > rows_per_batch ? buf_bytes : 1)) || (rc = c->dense_neg.ensure(8)))
            return rc;
        const int load_bytes = host::dense_load_bytes(wave_offset, row_bytes, es);
        unsigned long long* d_neg = c->dense_neg.as<unsigned long long>();
        // batch k: copied on the context's stream into buffer k & 1, unpacked on the second stream once the copy has
        // landed; the copy of batch k + 1 runs meanwhile, and batch k + 2 waits for this unpack before it reuses the buffer
        auto run = [&]() -> int {
            if (elem == WFA_DENSE_I16) WFA_HIP_CHECK(hipMemsetAsync(d_neg, 0xff, 8, c->dense_stream));
            int64_t k = 0;
            for (int64_t row = 0; row < n_rows; row += rows_per_batch, ++k) {
                const int64_t nr = std::min(rows_per_batch, n_rows - row);
                const int b = (int)(k & 1);
                if (k >= 2) WFA_HIP_CHECK(hipEventSynchronize(c->dense_ev[b]));
                if (int e = h2d_copy(c, c->dense_rows[b].ptr, (const uint8_t*)rows + (size_t)row * (size_t)row_bytes,
                                     (size_t)nr * (size_t)row_bytes))
                    return e;
                WFA_HIP_CHECK(hipEventRecord(c->dense_ev[2], c->stream));
                WFA_HIP_CHECK(hipStreamWaitEvent(c->dense_stream, c->dense_ev[2], 0));
                host::DenseBatch db{};
                db.out_begin = (uint64_t)row * (uint64_t)wave_length;
                db.out_end = (uint64_t)(row + nr) * (uint64_t)wave_length;
                db.row0 = row;
                db.L = (uint32_t)wave_length;
                db.row_elems = (uint32_t)(row_bytes / es);
                db.wave_elem = (uint32_t)(wave_offset / es);
                const uint8_t* src = c->dense_rows[b].as<uint8_t>();
                int e;
                if (elem == WFA_DENSE_I16) e = launch_dense_unpack<2, true>(load_bytes, c->dense_stream, src, pool.as<uint8_t>(), db, d_neg);
                else if (elem == WFA_DENSE_U16) e = launch_dense_unpack<2, false>(load_bytes, c->dense_stream, src, pool.as<uint8_t>(), db, d_neg);
                else e = launch_dense_unpack<4, false>(load_bytes, c->dense_stream, src, pool.as<uint8_t>(), db, d_neg);
                if (e) return e;
                WFA_HIP_CHECK(hipEventRecord(c->dense_ev[b], c->dense_stream));
            }
            return WFA_OK;
        };
        rc = run();
        // both streams are idle before anything is reported: the buffers and the events belong to the next call
        const hipError_t e0 = hipStreamSynchronize(c->stream), e1 = hipStreamSynchronize(c->dense_stream);
        if (rc) return rc;
        if (e0 != hipSuccess || e1 != hipSuccess)
            return fail(WFA_E_HIP, "dense upload failed: %s", hipGetErrorString(e0 != hipSuccess ? e0 : e1));
        if (elem == WFA_DENSE_I16) {
            unsigned long long neg = ~0ull;
            WFA_HIP_CHECK(hipMemcpy(&neg, d_neg, 8, hipMemcpyDeviceToHost));
            if (neg != ~0ull) {
                if (first_negative_row) *first_negative_row = (int64_t)neg;
                return fail(WFA_E_INVALID, "dense rows hold negative samples (first in row %lld)", (long long)neg);
            }
        }
    }
    pool_replaced(c, n, u16);
    return WFA_OK;
}

int wfa_upload_records_soa(wfa_ctx* c, int64_t R, const int64_t* off, const int32_t* len,
                           const double* baseline, const int8_t* pol, const double* thr,
                           const int64_t* ts, const int32_t* dt, const int16_t* board,
                           const int16_t* chan, const int64_t* rid) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!c->have_u16 && !c->have_f32) return fail(WFA_E_STATE, "upload a pool before the records");
    if (R < 0) return fail(WFA_E_INVALID, "negative record count");
    if (R > 0 && (!off || !len || !baseline || !pol || !thr || !ts || !dt || !board || !chan || !rid))
        return fail(WFA_E_INVALID, "null records column");
    int32_t max_len = 0;
    for (int64_t r = 0; r < R; ++r) {
        // same checks, same wording as data/records_view.py:47-56
        if (off[r] < 0) return fail(WFA_E_INVALID, "records contain negative wave_offset values");
        if (len[r] < 0) return fail(WFA_E_INVALID, "records contain negative event_length values");
        if (off[r] + (int64_t)len[r] > c->pool_n)
            return fail(WFA_E_INVALID, "records reference samples outside wave_pool bounds");
        if (len[r] > WFA_MAX_RECORD_SAMPLES)
            return fail(WFA_E_LIMIT, "record %lld has %d samples; this build supports at most %d",
                        (long long)r, len[r], WFA_MAX_RECORD_SAMPLES);
        if (pol[r] < WFA_POL_UNKNOWN || pol[r] > WFA_POL_POSITIVE_WAVE)
            return fail(WFA_E_INVALID, "bad polarity code %d at record %lld", (int)pol[r], (long long)r);
        if (len[r] > max_len) max_len = len[r];
    }
    // per-record region of the hit bitmap: bits indexed from the 16-byte aligned chunk base,
    // whole 64-bit words, one spare word
    std::vector<int64_t> bm_off((size_t)R);
    int64_t bm_total = 0;
    for (int64_t r = 0; r < R; ++r) {
        bm_off[(size_t)r] = bm_total;
        bm_total += ((int64_t)len[r] + 7 + 63) / 64 * 8 + 8;
    }
    const bool uniform = host::records_uniform(R, off, len, pol);
    const UniformLayout layout = host::uniform_layout(uniform, R, R ? len[0] : 0, R ? off[0] : 0, R ? pol[0] : 0, c->have_u16);
    const size_t n = (size_t)R;
    if ((rc = h2d(c, c->bm_off, bm_off.data(), n * 8))) return rc;
    if ((rc = h2d(c, c->off, off, n * 8))) return rc;
    if ((rc = h2d(c, c->len, len, n * 4))) return rc;
    if ((rc = h2d(c, c->baseline, baseline, n * 8))) return rc;
    if ((rc = h2d(c, c->pol, pol, n))) return rc;
    if ((rc = h2d(c, c->thr, thr, n * 8))) return rc;
    if ((rc = h2d(c, c->ts, ts, n * 8))) return rc;
    if ((rc = h2d(c, c->dt, dt, n * 4))) return rc;
    if ((rc = h2d(c, c->board, board, n * 2))) return rc;
    if ((rc = h2d(c, c->chan, chan, n * 2))) return rc;
    if ((rc = h2d(c, c->rid, rid, n * 8))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    records_replaced(c, R, max_len, bm_total + 64, layout);
    return WFA_OK;
}


int wfa_upload_records_packed(wfa_ctx* c, const void* rows, int64_t R, int32_t row_bytes, const int32_t* field_offsets,
                              int32_t polarity_chars, double threshold, const double* thresholds, const int8_t* polarity,
                              int32_t* max_len_out, int* record_ids_increasing) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!c->have_u16 && !c->have_f32) return fail(WFA_E_STATE, "upload a pool before the records");
    if (R < 0) return fail(WFA_E_INVALID, "negative record count");
    if (row_bytes <= 0 || !field_offsets || (R > 0 && !rows)) return fail(WFA_E_INVALID, "bad packed rows");
    PackedFields f{};
    int32_t* fo = &f.off;
    // order: wave_offset, event_length, baseline, polarity, timestamp, dt, board, channel, record_id
    const int32_t width[9] = {8, 4, 8, 4 * polarity_chars, 8, 4, 2, 2, 8};
    const bool required[9] = {true, true, true, false, true, false, false, false, true};
    for (int k = 0; k < 9; ++k) {
        fo[k] = field_offsets[k];
        if (fo[k] < 0 && required[k]) return fail(WFA_E_INVALID, "packed rows lack a required field (index %d)", k);
        if (fo[k] >= 0 && fo[k] + width[k] > row_bytes) return fail(WFA_E_INVALID, "field %d does not fit a %d-byte row", k, row_bytes);
    }
    if (f.polarity >= 0 && polarity_chars < 8) f.polarity = -1;  // neither "negative" nor "positive" fits: always unknown
    f.polarity_chars = polarity_chars;
    f.row_bytes = row_bytes;
    const size_t n = (size_t)R;
    if ((rc = c->off.ensure(n * 8)) || (rc = c->len.ensure(n * 4)) || (rc = c->baseline.ensure(n * 8)) || (rc = c->pol.ensure(n)) ||
        (rc = c->thr.ensure(n * 8)) || (rc = c->ts.ensure(n * 8)) || (rc = c->dt.ensure(n * 4)) || (rc = c->board.ensure(n * 2)) ||
        (rc = c->chan.ensure(n * 2)) || (rc = c->rid.ensure(n * 8)) || (rc = c->bm_off.ensure(n * 8)))
        return rc;
    records_dropped(c);  // from here on a failure leaves the context without records
    int32_t max_len = 0;
    bool increasing = true;
    int64_t bitmap_bytes = 64;
    UniformLayout layout;
    if (R > 0) {
        // scratch: the rows, per-record bitmap bytes, the optional per-record columns of the caller, the result block
        DevBuf d_rows, d_bm, d_thr, d_pol, d_res, d_blocks;
        const int64_t nb = scan_blocks_for(R);
        if ((rc = h2d(c, d_rows, rows, n * (size_t)row_bytes))) return rc;
        if ((rc = d_bm.ensure(n * 4)) || (rc = d_res.ensure(sizeof(UnpackResult))) || (rc = d_blocks.ensure((size_t)(nb + 1) * 8))) return rc;
        if (thresholds && (rc = h2d(c, d_thr, thresholds, n * 8))) return rc;
        if (polarity && (rc = h2d(c, d_pol, polarity, n))) return rc;
        UnpackResult init{};
        for (auto& x : init.first_bad) x = ~0ull;
        WFA_HIP_CHECK(hipMemcpyAsync(d_res.ptr, &init, sizeof(init), hipMemcpyHostToDevice, c->stream));
        RecView cols{};
        cols.baseline_rw = c->baseline.as<double>();
        {
            LaunchTimer t(c);
            hipLaunchKernelGGL(k_unpack_records, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, c->stream,
                               d_rows.as<uint8_t>(), R, f, c->pool_n, threshold, thresholds ? d_thr.as<double>() : nullptr,
                               polarity ? d_pol.as<int8_t>() : nullptr, cols, c->pol.as<int8_t>(), c->thr.as<double>(),
                               c->off.as<int64_t>(), c->len.as<int32_t>(), c->ts.as<int64_t>(), c->dt.as<int32_t>(),
                               c->board.as<int16_t>(), c->chan.as<int16_t>(), c->rid.as<int64_t>(), d_bm.as<int32_t>(),
                               d_res.as<UnpackResult>());
            WFA_HIP_CHECK(hipGetLastError());
            WFA_HIP_CHECK(launch_scan(c->stream, d_bm.as<int32_t>(), R, d_blocks.as<int64_t>(), c->bm_off.as<int64_t>()));
            if ((rc = t.end("k_unpack_records + bitmap offsets"))) return rc;
        }
        UnpackResult res{};
        int64_t bm_total = 0;
        int64_t off0 = 0;
        int32_t len0 = 0;
        int8_t pol0 = 0;
        WFA_HIP_CHECK(hipMemcpyAsync(&res, d_res.ptr, sizeof(res), hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipMemcpyAsync(&bm_total, d_blocks.as<int64_t>() + nb, 8, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipMemcpyAsync(&off0, c->off.ptr, 8, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipMemcpyAsync(&len0, c->len.ptr, 4, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipMemcpyAsync(&pol0, c->pol.ptr, 1, hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        // the earliest offending record decides, its checks in the order of the column route (records_view.py:47-56)
        unsigned long long worst = ~0ull;
        for (auto x : res.first_bad) worst = x < worst ? x : worst;
        if (worst != ~0ull) {
            if (res.first_bad[0] == worst) return fail(WFA_E_INVALID, "records contain negative wave_offset values");
            if (res.first_bad[1] == worst) return fail(WFA_E_INVALID, "records contain negative event_length values");
            if (res.first_bad[2] == worst) return fail(WFA_E_INVALID, "records reference samples outside wave_pool bounds");
            return fail(WFA_E_LIMIT, "record %lld has more samples than this build supports (at most %d)", (long long)worst,
                        WFA_MAX_RECORD_SAMPLES);
        }
        if (polarity) {  // caller's codes: range-checked like the column route (the kernel only compared them)
            for (int64_t r = 0; r < R; ++r)
                if (polarity[r] < WFA_POL_UNKNOWN || polarity[r] > WFA_POL_POSITIVE_WAVE)
                    return fail(WFA_E_INVALID, "bad polarity code %d at record %lld", (int)polarity[r], (long long)r);
        }
        max_len = res.max_len;
        increasing = res.rid_not_increasing == 0;
        bitmap_bytes = bm_total + 64;
        layout = host::uniform_layout(res.nonuniform == 0, R, len0, off0, pol0, c->have_u16);
    }
    records_replaced(c, R, max_len, bitmap_bytes, layout);
    if (max_len_out) *max_len_out = max_len;
    if (record_ids_increasing) *record_ids_increasing = increasing ? 1 : 0;
    return WFA_OK;
}

// validate a Savitzky-Golay plan and upload its tables into `s` (the context's plan, or a resident slot)
static int sg_plan_upload(wfa_ctx* c, SgPlanDev& s, int window, int polyorder, const double* tab, const uint8_t* symmetric,
                          int int_ok, const int32_t* itab, int32_t den, int32_t den_edge, int64_t guard,
                          int64_t guard_edge) {
    int rc;
    if (window < 1 || (window & 1) == 0 || window > WFA_MAX_SG_WINDOW)
        return fail(WFA_E_INVALID, "Savitzky-Golay window must be odd and in [1, %d], got %d",
                    WFA_MAX_SG_WINDOW, window);
    if (polyorder < 0 || polyorder >= window)
        return fail(WFA_E_INVALID, "polyorder %d must be in [0, window)", polyorder);
    if (!tab || !symmetric) return fail(WFA_E_INVALID, "null plan table");
    if (int_ok && (!itab || den <= 0 || den_edge <= 0)) return fail(WFA_E_INVALID, "bad integer plan");
    s.W = window; s.P = polyorder; s.H = window / 2;
    s.n_tables = (window + 1) / 2;
    s.stride = window + 2 * s.H * window;
    s.int_ok = int_ok ? 1 : 0;
    s.den = int_ok ? den : 1;
    s.den_edge = int_ok ? den_edge : 1;
    s.guard = guard; s.guard_edge = guard_edge;
    s.rden = 1.0 / (double)s.den;
    s.rden_edge = 1.0 / (double)s.den_edge;
    if ((rc = h2d(c, s.tab, tab, (size_t)s.n_tables * s.stride * sizeof(double)))) return rc;
    if ((rc = h2d(c, s.sym, symmetric, (size_t)s.n_tables))) return rc;
    const size_t isz = (size_t)s.stride * sizeof(int32_t);
    if (int_ok) {
        if ((rc = h2d(c, s.itab, itab, isz))) return rc;
    } else {
        if ((rc = s.itab.ensure(isz))) return rc;
    }
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_set_sg_plan(wfa_ctx* c, int window, int polyorder, const double* tab, const uint8_t* symmetric,
                    int int_ok, const int32_t* itab, int32_t den, int32_t den_edge, int64_t guard,
                    int64_t guard_edge) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = sg_plan_upload(c, c->sg, window, polyorder, tab, symmetric, int_ok, itab, den, den_edge, guard, guard_edge)))
        return rc;
    c->have_sg = true;
    return WFA_OK;
}

int wfa_sg_plan_store(wfa_ctx* c, int slot, int window, int polyorder, const double* tab, const uint8_t* symmetric,
                      int int_ok, const int32_t* itab, int32_t den, int32_t den_edge, int64_t guard,
                      int64_t guard_edge) {
    int rc = use_device(c);
    if (rc) return rc;
    if (slot < 0 || slot >= WFA_MAX_HIT_GROUPS)
        return fail(WFA_E_INVALID, "plan slot must be in [0, %d), got %d", WFA_MAX_HIT_GROUPS, slot);
    if (c->pending) {  // a queued pass may read the slot's tables
        int64_t n = 0;
        if ((rc = wfa_hits_wait(c, &n))) return rc;
    }
    c->have_slot[slot] = false;
    if ((rc = sg_plan_upload(c, c->sg_slot[slot], window, polyorder, tab, symmetric, int_ok, itab, den, den_edge, guard,
                             guard_edge)))
        return rc;
    c->have_slot[slot] = true;
    return WFA_OK;
}

int wfa_baseline_mean(wfa_ctx* c, int32_t start, int32_t end, int update_records, double* out) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, WFA_SRC_RAW))) return rc;
    if (start < 0) return fail(WFA_E_INVALID, "baseline window start must be >= 0");
    if (c->R == 0) return WFA_OK;
    const host::BaselineWindow w = host::baseline_window(start, end, c->max_len);
    start = w.start; end = w.end;
    double* dst = c->baseline.as<double>();
    if (!update_records) {
        if ((rc = c->out_rows.ensure((size_t)c->R * sizeof(double)))) return rc;
        dst = c->out_rows.as<double>();
    }
    {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_baseline_mean(c->stream, pool_view(c), rec_view(c), start, end, dst));
        if ((rc = t.end("k_baseline_mean"))) return rc;
    }
    if (out)
        WFA_HIP_CHECK(hipMemcpyAsync(out, dst, (size_t)c->R * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_filter_keep_output(wfa_ctx* c, int keep) {
    int rc = use_device(c);
    if (rc) return rc;
    if (keep && (!c->have_f32 || c->pool_f32.cap < (size_t)c->pool_n * sizeof(float)))
        return fail(WFA_E_STATE, "keep requested but no filtered output exists yet");
    c->filter_keep = keep != 0;
    return WFA_OK;
}

int wfa_download_pool_f32(wfa_ctx* c, float* out, int64_t n) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!c->have_f32) return fail(WFA_E_STATE, "no float32 pool is resident");
    if (n != c->pool_n) return fail(WFA_E_INVALID, "caller expects %lld samples, the pool has %lld", (long long)n, (long long)c->pool_n);
    if (n == 0) return WFA_OK;
    if (!out) return fail(WFA_E_INVALID, "out is null");
    WFA_HIP_CHECK(hipMemcpyAsync(out, c->pool_f32.ptr, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_download_pool_f32_range(wfa_ctx* c, float* out, int64_t start, int64_t n) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!c->have_f32) return fail(WFA_E_STATE, "no float32 pool is resident");
    if (start < 0 || n < 0 || start > c->pool_n || n > c->pool_n - start)
        return fail(WFA_E_INVALID, "samples [%lld, %lld + %lld) are outside the pool of %lld", (long long)start,
                    (long long)start, (long long)n, (long long)c->pool_n);
    if (n == 0) return WFA_OK;
    if (!out) return fail(WFA_E_INVALID, "out is null");
    WFA_HIP_CHECK(hipMemcpyAsync(out, c->pool_f32.as<float>() + start, (size_t)n * sizeof(float),
                                 hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

// K2 over the uploaded records (c->R > 0) under `plan`, into the float32 pool: the span kernel on uniform records, else
// one wave per record.  sel (device, one int32 per record) != nullptr: only the records r with sel[r] == group
// (wfa_savgol_group); the route is chosen from the layout of the whole table either way.
static int savgol_launch(wfa_ctx* c, const SgPlanDev* plan, const int32_t* sel, int32_t group) {
    int rc;
    const SgParams sp0 = sg_params(plan);
    const UniformLayout& u = c->layout;
    const bool fast = sg_mask_supported(sp0) && !c->opt.no_fast;
    // uniform records, L % 16 != 0: the span kernel reads the padded shadow and writes the packed pool
    const bool padded = u.pad && u.L >= sp0.W && fast && !c->opt.no_pad;
    LayoutView v;
    if ((rc = layout_view(c, c->thr.as<double>(), padded, &v))) return rc;
    LaunchTimer t(c);
    if (padded || (u.span && u.L >= 16 && u.L >= sp0.W && fast)) {
        SpanParams sp{};
        sp.off0 = v.off0; sp.L = v.L; sp.positive = 0;
        if (padded) { sp.S = v.S; sp.out_off0 = u.off0; }
        sp.rs = 64;
        sp.n_spans = (c->R + sp.rs - 1) / sp.rs;
        // (the records as uploaded: their offsets address the output)
        WFA_HIP_CHECK(launch_savgol_span(c->stream, v.pool, rec_view(c), sp0, sp, c->pool_f32.as<float>(), sel, group));
        if (sel) return t.end(padded ? "k_savgol_span<padded, group>" : "k_savgol_span<group>");
        return t.end(padded ? "k_savgol_span<padded>" : "k_savgol_span");
    }
    WFA_HIP_CHECK(launch_savgol(c->stream, v.pool, v.rec, sp0, c->pool_f32.as<float>(), sel, group));
    return t.end(sel ? "k_savgol<group>" : "k_savgol");
}

int wfa_savgol(wfa_ctx* c, float* out) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, WFA_SRC_SG_FUSED))) return rc;
    if ((rc = c->pool_f32.ensure((size_t)c->pool_n * sizeof(float)))) return rc;
    // gaps between records stay 0.0 (records.py:382)
    if (!c->filter_keep) WFA_HIP_CHECK(hipMemsetAsync(c->pool_f32.ptr, 0, (size_t)c->pool_n * sizeof(float), c->stream));
    if (c->R > 0 && (rc = savgol_launch(c, ctx_plan(c), nullptr, 0))) return rc;
    c->have_f32 = true;
    if (out)
        WFA_HIP_CHECK(hipMemcpyAsync(out, c->pool_f32.ptr, (size_t)c->pool_n * sizeof(float),
                                     hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_sosfiltfilt(wfa_ctx* c, int n_sections, const double* sos, const double* zi, int32_t padlen, float* out) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, WFA_SRC_RAW))) return rc;
    if (n_sections < 1 || n_sections > WFA_MAX_SOS_SECTIONS)
        return fail(WFA_E_INVALID, "n_sections must be in [1, %d], got %d", WFA_MAX_SOS_SECTIONS, n_sections);
    if (!sos || !zi || padlen < 0) return fail(WFA_E_INVALID, "bad sosfiltfilt arguments");
    if ((rc = c->pool_f32.ensure((size_t)c->pool_n * sizeof(float)))) return rc;
    if (!c->filter_keep) WFA_HIP_CHECK(hipMemsetAsync(c->pool_f32.ptr, 0, (size_t)c->pool_n * sizeof(float), c->stream));
    if (c->R > 0) {
        // forward-pass scratch: [max_len + 2 padlen][batch] float64, batches bounded to ~2 GiB
        const int64_t n_ext = (int64_t)c->max_len + 2 * (int64_t)padlen;
        int64_t batch = (int64_t)(2147483648LL / (n_ext * 8));
        batch = batch / 256 * 256;
        if (batch < 256) batch = 256;
        if (batch > c->R) batch = (c->R + 255) / 256 * 256;
        if ((rc = c->bw_scratch.ensure((size_t)(n_ext * batch * 8)))) return rc;
        const PoolView pv = pool_view(c);
        const RecView rv = rec_view(c);
        LaunchTimer t(c);
        for (int64_t r0 = 0; r0 < c->R; r0 += batch) {
            const int64_t r1 = r0 + batch < c->R ? r0 + batch : c->R;
            WFA_HIP_CHECK(launch_sosfiltfilt(c->stream, pv, rv, n_sections, sos, zi, padlen, r0, r1,
                                             c->bw_scratch.as<double>(), batch, c->pool_f32.as<float>()));
        }
        if ((rc = t.end("k_sosfiltfilt"))) return rc;
    }
    c->have_f32 = true;
    if (out)
        WFA_HIP_CHECK(hipMemcpyAsync(out, c->pool_f32.ptr, (size_t)c->pool_n * sizeof(float), hipMemcpyDeviceToHost,
                                     c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_threshold_hits_count(wfa_ctx* c, int source, int32_t le, int32_t re, int32_t max_len,
                             int64_t* n_hits) {
    return ctx_pass(c, source, false, 0, 0, le, re, max_len, n_hits, false);
}

int wfa_fused_baseline_filter_hits(wfa_ctx* c, int32_t bl_start, int32_t bl_end, int32_t le, int32_t re,
                                   int32_t max_len, int64_t* n_hits) {
    return ctx_pass(c, WFA_SRC_SG_FUSED, bl_end > bl_start, bl_start, bl_end, le, re, max_len, n_hits, false);
}

int wfa_hits_enqueue(wfa_ctx* c, int source, int32_t bl_start, int32_t bl_end, int32_t le, int32_t re, int32_t max_len) {
    return ctx_pass(c, source, source == WFA_SRC_SG_FUSED && bl_end > bl_start, bl_start, bl_end, le, re, max_len,
                    nullptr, true);
}

int wfa_hits_wait(wfa_ctx* c, int64_t* n_hits) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!n_hits) return fail(WFA_E_INVALID, "n_hits is null");
    if (c->pending == wfa_ctx::kPendGroups) return groups_wait(c, n_hits);
    if (c->pending) {
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        c->pending = wfa_ctx::kPendNone;
        int64_t total = 0;
        if (!pass_settle(c, c->pend.out.bound, c->pend.out.runs32, &total)) {  // redone the exact way, now
            const HitPass p = c->pend.pass;  // (its arguments; plan, thresholds and hint as the context holds them now)
            return ctx_pass(c, p.source, p.fused_bl, p.bl_start, p.bl_end, p.le, p.re, p.max_len, n_hits, false);
        }
        c->n_hits = total;
    }
    if (c->n_hits < 0) return fail(WFA_E_STATE, "no hit pass has been run");
    *n_hits = c->n_hits;
    return WFA_OK;
}

int wfa_threshold_hits_fill(wfa_ctx* c, void* out_rows, int64_t n_hits) {
    int rc = use_device(c);
    if (rc) return rc;
    if (c->pending) {
        int64_t n = 0;
        if ((rc = wfa_hits_wait(c, &n))) return rc;
    }
    if (c->n_hits < 0) return fail(WFA_E_STATE, "no hit pass has been run");
    if (n_hits != c->n_hits)
        return fail(WFA_E_INVALID, "caller expects %lld rows, the pass produced %lld", (long long)n_hits,
                    (long long)c->n_hits);
    if (n_hits == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->hit_out.ptr, (size_t)n_hits * 60, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

}  // extern "C"

// ---- the grouped pass: one pass per filter group, the rows merged into one table (wfa_hits_enqueue_groups) ----------
// The passes run over the same uploaded records with thresholds that leave every record to one of them (per-channel
// filter settings: cpu/filtering.py:339-374 resolved per record, hit_finder.py:288-327 for the thresholds); the reference
// finds the hits of all records in one loop and so emits them by (record index, start) (hit_finder.py:354-366).  Every
// pass is stashed as it is -- its 60-byte rows and the record index of each -- and the merge is a per-record row
// count, an exclusive scan over the records and a scatter of the rows.  `rec` of one pass ascends, so the rows of a
// record inside a pass are found by binary search.
constexpr int kMergeBlock = 256;

// which pass (set) row i belongs to: sets[0] = 0 <= ... <= sets[G] = n (empty passes repeat a boundary)
__device__ __forceinline__ int merge_set_of(const int64_t* __restrict__ sets, int G, int64_t i) {
    int g = 0;
    while (g + 1 < G && sets[g + 1] <= i) ++g;
    return g;
}

// first index in [lo, hi) whose record is >= r (Upper: > r)
template <bool Upper>
__device__ __forceinline__ int64_t merge_bound(const int32_t* __restrict__ rec, int64_t lo, int64_t hi, int32_t r) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int32_t v = rec[mid];
        if (Upper ? v <= r : v < r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// per-record row count over all passes: the first row of a record inside a pass adds that pass's rows of the record
__global__ __launch_bounds__(kMergeBlock) void k_hit_rows_merge_count(int64_t n, const int32_t* __restrict__ rec,
                                                                      const int64_t* __restrict__ sets, int G, int64_t R,
                                                                      int32_t* __restrict__ counts,
                                                                      const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (n_dev && *n_dev < n) n = *n_dev;  // launched for a bound: the total stands on the device
    if (i >= n) return;
    const int g = merge_set_of(sets, G, i);
    const int32_t r = rec[i];
    if (r < 0 || r >= R) return;
    if (i > sets[g] && rec[i - 1] == r) return;
    const int64_t end = merge_bound<true>(rec, i, sets[g + 1], r);
    atomicAdd(&counts[r], (int32_t)(end - i));
}

// final place of every row: first row of its record, + the record's rows in earlier passes, + its rank inside its own pass
__global__ __launch_bounds__(kMergeBlock) void k_hit_rows_merge_place(int64_t n, const int32_t* __restrict__ rec,
                                                                      const int64_t* __restrict__ sets, int G, int64_t R,
                                                                      const int64_t* __restrict__ out_start,
                                                                      int64_t* __restrict__ dest,
                                                                      const int64_t* __restrict__ n_dev) {
    const int64_t i = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (n_dev && *n_dev < n) n = *n_dev;
    if (i >= n) return;
    const int g = merge_set_of(sets, G, i);
    const int32_t r = rec[i];
    if (r < 0 || r >= R) { dest[i] = -1; return; }
    int64_t pos = out_start[r] + (i - merge_bound<false>(rec, sets[g], i, r));
    for (int e = 0; e < g; ++e) {
        const int64_t lo = merge_bound<false>(rec, sets[e], sets[e + 1], r);
        pos += merge_bound<true>(rec, lo, sets[e + 1], r) - lo;
    }
    dest[i] = pos;
}

// 60-byte rows as 15 dwords: consecutive lanes read consecutive dwords of the stash and write runs of 15 into the table
__global__ __launch_bounds__(kMergeBlock) void k_hit_rows_merge_scatter(int64_t n, const uint32_t* __restrict__ src,
                                                                        const int64_t* __restrict__ dest,
                                                                        uint32_t* __restrict__ out,
                                                                        const int64_t* __restrict__ n_dev) {
    const int64_t d = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (n_dev && *n_dev < n) n = *n_dev;
    if (d >= n * 15) return;
    const int64_t i = d / 15;
    const int64_t to = dest[i];
    if (to < 0 || to >= n) return;
    out[to * 15 + (d - i * 15)] = src[d];
}

static unsigned merge_grid(int64_t n) { return (unsigned)((n + kMergeBlock - 1) / kMergeBlock); }

// grow a stash buffer to `want` bytes and keep its first `used` bytes (DevBuf::ensure drops the contents)
static int merge_grow(wfa_ctx* c, DevBuf& b, size_t used, size_t want) {
    if (want <= b.cap) return WFA_OK;
    if (used == 0) return b.ensure(want);
    want = std::max(want, 2 * b.cap);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want + 256);
    if (e != hipSuccess) return fail(WFA_E_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    e = hipMemcpyAsync(p, b.ptr, used, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(WFA_E_HIP, "growing the merge stash failed: %s", hipGetErrorString(e));
    }
    (void)hipFree(b.ptr);
    b.ptr = p;
    b.cap = want;
    return WFA_OK;
}

// Everything is queued on the context's stream: per group a kernel writes the own-or-+inf copy of the threshold column
// (grp_thr) from group_of_record, the single pass is queued on that copy under the plan of the group's resident slot
// (run_hits, enqueue_only), one thread takes the pass's row count where the pass reported it (the pinned words of a queued
// pass, or the count the host already holds) and writes the group's stash offset, and a copy kernel launched for the
// pass's row bound moves that many rows and record indices to the stash.  The merge kernels are launched for the sum of
// the bounds and read the total from the last stash offset.  The context's own plan, thresholds and options are only read.
//
// Pinned block (int64 words): per group (rows, overflow flags) of its pass, the stash offsets as the device wrote them
// ([n_groups] = the merged row count), the fail flag (a group outgrew its bound, its events or the stash).
constexpr int kGrpSets = 2 * WFA_MAX_HIT_GROUPS;
constexpr int kGrpFail = kGrpSets + WFA_MAX_HIT_GROUPS + 1;
constexpr int kGrpWords = 32;
constexpr int kGrpFailDev = WFA_MAX_HIT_GROUPS + 1;  // grp_sets: [0, WFA_MAX_HIT_GROUPS] stash offsets, then the fail flag
static_assert(kGrpFail < kGrpWords, "pinned block of the grouped pass");

__global__ __launch_bounds__(kMergeBlock) void k_grp_mask(int64_t R, const int32_t* __restrict__ group_of_record, int32_t g,
                                                          const double* __restrict__ own, double* __restrict__ thr) {
    const int64_t r = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (r >= R) return;
    thr[r] = group_of_record[r] == g ? own[r] : __longlong_as_double(0x7ff0000000000000ll);  // +inf: no hit on any route
}

// One thread, behind group g's pass: its row count (n_host >= 0: the host read it; otherwise the words the queued pass
// reported to pinned memory), whether its speculative launch stands, and the stash offset of the next group.
__global__ void k_grp_take(int g, int64_t n_host, int runs32, int64_t bound, int64_t cap_rows,
                           const volatile int64_t* pass_report, int64_t* sets, volatile int64_t* h) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t n = n_host, flags = 0;
    if (n_host < 0) {
        n = pass_report[0];
        if (runs32) flags = pass_report[2] & 0xffffffffll;
    }
    bool ok = n_host >= 0 || (n >= 0 && n <= bound && flags == 0);
    if (g == 0) { sets[0] = 0; sets[kGrpFailDev] = 0; }
    const int64_t at = g == 0 ? 0 : sets[g];
    int64_t take = ok ? n : 0;
    if (at + take > cap_rows) { take = 0; ok = false; }
    if (!ok) sets[kGrpFailDev] = 1;
    sets[g + 1] = at + take;
    h[2 * g] = n;
    h[2 * g + 1] = flags;
    h[kGrpSets + g + 1] = at + take;
    h[kGrpFail] = sets[kGrpFailDev];
}

// Rows of group g's pass into the stash, 15 dwords per row, and the record index of every row.  desc != null: the run
// descriptors of the streaming / bitmap routes; otherwise the general route's exclusive scan of the per-record counts (row
// d belongs to the last record whose first row is <= d: the records behind it without a hit start past d).  Launched for
// the pass's row bound; the count stands in sets[].
__global__ __launch_bounds__(kMergeBlock) void k_grp_stash(int g, const int64_t* __restrict__ sets,
                                                           const uint32_t* __restrict__ rows, const int4* __restrict__ desc,
                                                           const int64_t* __restrict__ out_start, int64_t R,
                                                           uint32_t* __restrict__ stash_rows, int32_t* __restrict__ stash_rec) {
    const int64_t at = sets[g], n = sets[g + 1] - at;
    const int64_t d = (int64_t)blockIdx.x * kMergeBlock + threadIdx.x;
    if (d >= n * 15) return;
    stash_rows[at * 15 + d] = rows[d];
    if (d >= n) return;
    if (desc) { stash_rec[at + d] = desc[d].x; return; }
    int64_t lo = 0, hi = R;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (out_start[mid] <= d) lo = mid + 1; else hi = mid;
    }
    stash_rec[at + d] = (int32_t)(lo - 1);
}

static int groups_pinned(wfa_ctx* c) {
    if (c->h_grp) return WFA_OK;
    const size_t bytes = kGrpWords * sizeof(int64_t) + WFA_MAX_HIT_GROUPS * sizeof(RunsCold);
    WFA_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c->h_grp), bytes, hipHostMallocDefault));
    memset(c->h_grp, 0, bytes);
    c->h_grp_cold = reinterpret_cast<RunsCold*>(c->h_grp + kGrpWords);
    return WFA_OK;
}

// One pass of the grouped call: group g's plan from its resident slot, the call's baseline window (SG groups), `thr` the
// column it compares against, the group's own hint and pinned cold block.  exact: no hint, no speculative launch.
static int groups_one_pass(wfa_ctx* c, int g, const double* thr, bool exact, HitOutcome* o) {
    const wfa_ctx::GroupsPass& G = c->grp;
    const bool sg = G.groups[g].source == WFA_SRC_SG_FUSED;
    HitPass p;
    p.source = G.groups[g].source;
    p.plan = sg ? &c->sg_slot[G.groups[g].plan_slot] : nullptr;
    p.thr = thr;
    p.fused_bl = sg && G.bl_end > G.bl_start;  // (WFA_SRC_F32 reads the uploaded baselines, as in wfa_hits_enqueue)
    p.bl_start = G.bl_start; p.bl_end = G.bl_end; p.le = G.le; p.re = G.re; p.max_len = G.max_len;
    p.hint = exact ? -1 : G.last[g];
    p.speculate = !exact && !c->opt.no_speculate;
    p.enqueue_only = true;
    p.cold_pin = c->h_grp_cold + g;  // (rewritten only when the plan's or the pool's buffers moved: a warm call waits for nothing)
    return run_hits(c, p, o);
}

// exact: every pass with the host round trip for its count (the redo of wfa_hits_wait; nothing stays pending).  The
// groups' outcomes are collected in c->grp; what the context remembers of the call is set once, at the end.
static int groups_run(wfa_ctx* c, bool exact) {
    wfa_ctx::GroupsPass& G = c->grp;
    const int n = G.n_groups;
    const int64_t R = c->R;
    int rc;
    HitOutcome o;
    if (G.single) {
        if ((rc = groups_one_pass(c, 0, c->thr.as<double>(), exact, &o))) return rc;
        if (o.state == HitOutcome::kQueued) {
            G.bound[0] = o.bound;
            G.runs32[0] = o.runs32;
            c->pending = wfa_ctx::kPendGroups;
        } else {
            c->n_hits = c->last_hits = G.last[0] = o.n_hits;
        }
        return WFA_OK;
    }
    auto planned = [&](int g) { return !exact && G.last[g] >= 0 ? rows_bound(G.last[g]) : (int64_t)0; };
    int64_t plan_rows = 0;
    for (int g = 0; g < n; ++g) plan_rows += planned(g);
    if ((rc = c->merge_rows.ensure((size_t)plan_rows * 60)) || (rc = c->merge_rec.ensure((size_t)plan_rows * sizeof(int32_t))) ||
        (rc = c->grp_thr.ensure((size_t)R * sizeof(double))) || (rc = c->grp_sets.ensure(16 * sizeof(int64_t))))
        return rc;
    int64_t* sets = c->grp_sets.as<int64_t>();
    int64_t n_bound = 0;  // rows the merge kernels are launched for
    bool queued = false;
    for (int g = 0; g < n; ++g) {
        {  // (one stream: the kernels of group g - 1 have read grp_thr before this one rewrites it)
            LaunchTimer t(c);
            hipLaunchKernelGGL(k_grp_mask, dim3(merge_grid(R)), dim3(kMergeBlock), 0, c->stream, R, c->grp_gor.as<int32_t>(),
                               (int32_t)g, c->thr.as<double>(), c->grp_thr.as<double>());
            if (hipGetLastError() != hipSuccess) return fail(WFA_E_HIP, "k_grp_mask launch failed");
            if ((rc = t.end("k_grp_mask"))) return rc;
        }
        if ((rc = groups_one_pass(c, g, c->grp_thr.as<double>(), exact, &o))) return rc;
        int64_t launch_rows;
        if (o.state == HitOutcome::kQueued) {  // its count is on its way to the pinned words of the single pass
            queued = true;
            G.bound[g] = o.bound;
            G.runs32[g] = o.runs32;
            G.n_host[g] = -1;
            launch_rows = G.bound[g];
        } else {  // ran to completion, the stream is idle: every earlier stash offset has reached the pinned block
            G.n_host[g] = G.last[g] = o.n_hits;
            G.bound[g] = o.n_hits;
            G.runs32[g] = false;
            launch_rows = o.n_hits;
            const int64_t at = g == 0 ? 0 : c->h_grp[kGrpSets + g];
            int64_t later = 0;
            for (int e = g + 1; e < n; ++e) later += planned(e);
            const int64_t want = at + launch_rows + later;
            if ((rc = merge_grow(c, c->merge_rows, (size_t)at * 60, (size_t)want * 60)) ||
                (rc = merge_grow(c, c->merge_rec, (size_t)at * sizeof(int32_t), (size_t)want * sizeof(int32_t))))
                return rc;
        }
        const int64_t cap_rows = (int64_t)std::min(c->merge_rows.cap / 60, c->merge_rec.cap / sizeof(int32_t));
        LaunchTimer t(c);
        hipLaunchKernelGGL(k_grp_take, dim3(1), dim3(64), 0, c->stream, g, G.n_host[g], G.runs32[g] ? 1 : 0, G.bound[g], cap_rows,
                           (const volatile int64_t*)c->h_total, sets, (volatile int64_t*)c->h_grp);
        if (launch_rows > 0 && c->rows_index != 0)
            hipLaunchKernelGGL(k_grp_stash, dim3(merge_grid(launch_rows * 15)), dim3(kMergeBlock), 0, c->stream, g, sets,
                               c->hit_out.as<uint32_t>(), c->rows_index == 1 ? c->hit_desc.as<int4>() : nullptr,
                               c->rec_out_start.as<int64_t>(), R, c->merge_rows.as<uint32_t>(), c->merge_rec.as<int32_t>());
        if (hipGetLastError() != hipSuccess) return fail(WFA_E_HIP, "k_grp_stash launch failed");
        if ((rc = t.end("k_grp_take + k_grp_stash"))) return rc;
        n_bound += launch_rows;
    }
    c->rows_index = 0;
    c->n_hits = -1;
    if (n_bound > 0) {
        const int64_t nb = scan_blocks_for(R);
        const int64_t room = rows_bound(n_bound);  // head room: the next call's bounds fit without a reallocation
        if (c->hit_out.cap < (size_t)n_bound * 60 || c->hit_desc.cap < (size_t)n_bound * sizeof(int4) ||
            c->merge_dest.cap < (size_t)n_bound * sizeof(int64_t)) {
            if (hipStreamSynchronize(c->stream) != hipSuccess)  // the stash kernels read the buffers that are about to move
                return fail(WFA_E_HIP, "waiting for the stash of the grouped pass failed");
            if ((rc = c->hit_out.ensure((size_t)room * 60)) || (rc = c->hit_desc.ensure((size_t)room * sizeof(int4))) ||
                (rc = c->merge_dest.ensure((size_t)room * sizeof(int64_t))))
                return rc;
        }
        if ((rc = c->rec_nhits.ensure((size_t)R * sizeof(int32_t))) || (rc = c->rec_out_start.ensure((size_t)R * sizeof(int64_t))) ||
            (rc = c->scan_blocks.ensure((size_t)(nb + 1) * sizeof(int64_t))))
            return rc;
        const int32_t* rec = c->merge_rec.as<int32_t>();
        int32_t* counts = c->rec_nhits.as<int32_t>();
        const int64_t* total = sets + n;
        if (hipMemsetAsync(counts, 0, (size_t)R * sizeof(int32_t), c->stream) != hipSuccess)
            return fail(WFA_E_HIP, "clearing the merge counts failed");
        {
            LaunchTimer t(c);
            hipLaunchKernelGGL(k_hit_rows_merge_count, dim3(merge_grid(n_bound)), dim3(kMergeBlock), 0, c->stream, n_bound, rec,
                               (const int64_t*)sets, n, R, counts, total);
            if (hipGetLastError() != hipSuccess) return fail(WFA_E_HIP, "k_hit_rows_merge_count launch failed");
            if ((rc = t.end("k_hit_rows_merge_count"))) return rc;
        }
        {
            LaunchTimer t(c);
            if (launch_scan(c->stream, counts, R, c->scan_blocks.as<int64_t>(), c->rec_out_start.as<int64_t>()) != hipSuccess)
                return fail(WFA_E_HIP, "k_scan(merged hit counts) launch failed");
            if ((rc = t.end("k_scan(merged hit counts)"))) return rc;
        }
        {
            LaunchTimer t(c);
            hipLaunchKernelGGL(k_hit_rows_merge_place, dim3(merge_grid(n_bound)), dim3(kMergeBlock), 0, c->stream, n_bound, rec,
                               (const int64_t*)sets, n, R, c->rec_out_start.as<int64_t>(), c->merge_dest.as<int64_t>(), total);
            if (hipGetLastError() != hipSuccess) return fail(WFA_E_HIP, "k_hit_rows_merge_place launch failed");
            if ((rc = t.end("k_hit_rows_merge_place"))) return rc;
        }
        {
            LaunchTimer t(c);
            hipLaunchKernelGGL(k_hit_rows_merge_scatter, dim3(merge_grid(n_bound * 15)), dim3(kMergeBlock), 0, c->stream, n_bound,
                               c->merge_rows.as<uint32_t>(), c->merge_dest.as<int64_t>(), c->hit_out.as<uint32_t>(), total);
            if (hipGetLastError() != hipSuccess) return fail(WFA_E_HIP, "k_hit_rows_merge_scatter launch failed");
            if ((rc = t.end("k_hit_rows_merge_scatter"))) return rc;
        }
    }
    if (queued) {  // wfa_hits_wait reads the pinned block
        c->pending = wfa_ctx::kPendGroups;
        return WFA_OK;
    }
    int64_t total = 0;
    for (int g = 0; g < n; ++g) total += G.n_host[g];
    c->n_hits = c->last_hits = total;
    return WFA_OK;
}

static int groups_wait(wfa_ctx* c, int64_t* n_hits) {
    wfa_ctx::GroupsPass& G = c->grp;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->pending = wfa_ctx::kPendNone;
    bool redo = false;
    if (G.single) {  // the single pass under the slot's plan: settled like wfa_hits_wait's own
        int64_t total = 0;
        redo = !pass_settle(c, G.bound[0], G.runs32[0], &total);
        G.last[0] = total;
        if (!redo) c->n_hits = total;
    } else {
        for (int g = 0; g < G.n_groups; ++g) {
            if (G.n_host[g] >= 0) continue;
            if (c->h_grp[2 * g + 1]) c->no_runs32 = true;  // a span outgrew its events: the general route from now on
            G.last[g] = c->h_grp[2 * g];
        }
        redo = c->h_grp[kGrpFail] != 0;
        if (!redo) c->n_hits = c->last_hits = c->h_grp[kGrpSets + G.n_groups];
    }
    if (redo) {
        if (!c->have_records || c->R != G.R)
            return fail(WFA_E_STATE, "the queued grouped pass must be redone, but its records table has been replaced");
        if (int rc = groups_run(c, true)) return rc;
    }
    *n_hits = c->n_hits;
    return WFA_OK;
}

extern "C" {

int wfa_sosfiltfilt_group(wfa_ctx* c, int n_sections, const double* sos, const double* zi, int32_t padlen,
                          const int32_t* group_of_record, int32_t group) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, WFA_SRC_RAW))) return rc;
    if (n_sections < 1 || n_sections > WFA_MAX_SOS_SECTIONS)
        return fail(WFA_E_INVALID, "n_sections must be in [1, %d], got %d", WFA_MAX_SOS_SECTIONS, n_sections);
    if (!sos || !zi || padlen < 0) return fail(WFA_E_INVALID, "bad sosfiltfilt arguments");
    if (c->R > 0 && !group_of_record) return fail(WFA_E_INVALID, "group_of_record is null");
    if (c->pending) {  // a queued pass may read the twin
        int64_t n = 0;
        if ((rc = wfa_hits_wait(c, &n))) return rc;
    }
    const bool fresh = !c->have_f32 || c->pool_f32.cap < (size_t)c->pool_n * sizeof(float);
    if ((rc = c->pool_f32.ensure((size_t)c->pool_n * sizeof(float)))) return rc;
    // a twin that did not exist: gaps and the other groups' records read 0.0 until their own filter call
    if (fresh) WFA_HIP_CHECK(hipMemsetAsync(c->pool_f32.ptr, 0, (size_t)c->pool_n * sizeof(float), c->stream));
    if (c->R > 0) {
        if ((rc = c->grp_gor.ensure((size_t)c->R * sizeof(int32_t)))) return rc;
        if ((rc = h2d_copy(c, c->grp_gor.ptr, group_of_record, (size_t)c->R * sizeof(int32_t)))) return rc;
        const int64_t n_ext = (int64_t)c->max_len + 2 * (int64_t)padlen;
        int64_t batch = (int64_t)(2147483648LL / (n_ext * 8));
        batch = batch / 256 * 256;
        if (batch < 256) batch = 256;
        if (batch > c->R) batch = (c->R + 255) / 256 * 256;
        if ((rc = c->bw_scratch.ensure((size_t)(n_ext * batch * 8)))) return rc;
        const PoolView pv = pool_view(c);
        const RecView rv = rec_view(c);
        LaunchTimer t(c);
        for (int64_t r0 = 0; r0 < c->R; r0 += batch) {
            const int64_t r1 = r0 + batch < c->R ? r0 + batch : c->R;
            WFA_HIP_CHECK(launch_sosfiltfilt(c->stream, pv, rv, n_sections, sos, zi, padlen, r0, r1,
                                             c->bw_scratch.as<double>(), batch, c->pool_f32.as<float>(),
                                             c->grp_gor.as<int32_t>(), group));
        }
        if ((rc = t.end("k_sosfiltfilt<group>"))) return rc;
    }
    c->have_f32 = true;
    return WFA_OK;
}

int wfa_savgol_group(wfa_ctx* c, int slot, const int32_t* group_of_record, int32_t group) {
    int rc = use_device(c);
    if (rc) return rc;
    if (slot < 0 || slot >= WFA_MAX_HIT_GROUPS)
        return fail(WFA_E_INVALID, "plan slot must be in [0, %d), got %d", WFA_MAX_HIT_GROUPS, slot);
    if (!c->have_records) return fail(WFA_E_STATE, "records not uploaded");
    if (!c->have_u16) return fail(WFA_E_STATE, "wave_pool (uint16) not uploaded");
    if (!c->have_slot[slot]) return fail(WFA_E_STATE, "plan slot %d holds no plan (wfa_sg_plan_store)", slot);
    if (c->R > 0 && !group_of_record) return fail(WFA_E_INVALID, "group_of_record is null");
    if (c->pending) {  // a queued pass may read the twin
        int64_t n = 0;
        if ((rc = wfa_hits_wait(c, &n))) return rc;
    }
    const bool fresh = !c->have_f32 || c->pool_f32.cap < (size_t)c->pool_n * sizeof(float);
    if ((rc = c->pool_f32.ensure((size_t)c->pool_n * sizeof(float)))) return rc;
    // a twin that did not exist: gaps and the other groups' records read 0.0 until their own filter call
    if (fresh) WFA_HIP_CHECK(hipMemsetAsync(c->pool_f32.ptr, 0, (size_t)c->pool_n * sizeof(float), c->stream));
    if (c->R > 0) {
        if ((rc = c->grp_gor.ensure((size_t)c->R * sizeof(int32_t)))) return rc;
        if ((rc = h2d_copy(c, c->grp_gor.ptr, group_of_record, (size_t)c->R * sizeof(int32_t)))) return rc;
        if ((rc = savgol_launch(c, &c->sg_slot[slot], c->grp_gor.as<int32_t>(), group))) return rc;
    }
    c->have_f32 = true;
    return WFA_OK;
}

int wfa_hits_enqueue_groups(wfa_ctx* c, int n_groups, const wfa_hit_group* groups, const int32_t* group_of_record,
                            int32_t bl_start, int32_t bl_end, int32_t le, int32_t re, int32_t max_len) {
    int rc = use_device(c);
    if (rc) return rc;
    if (n_groups < 1 || n_groups > WFA_MAX_HIT_GROUPS)
        return fail(WFA_E_INVALID, "n_groups must be in [1, %d], got %d", WFA_MAX_HIT_GROUPS, n_groups);
    if (!groups) return fail(WFA_E_INVALID, "groups is null");
    if (!c->have_records) return fail(WFA_E_STATE, "records not uploaded");
    if (!c->have_u16) return fail(WFA_E_STATE, "wave_pool (uint16) not uploaded");
    for (int g = 0; g < n_groups; ++g) {
        if (groups[g].source == WFA_SRC_SG_FUSED) {
            const int slot = groups[g].plan_slot;
            if (slot < 0 || slot >= WFA_MAX_HIT_GROUPS)
                return fail(WFA_E_INVALID, "group %d: plan slot must be in [0, %d), got %d", g, WFA_MAX_HIT_GROUPS, slot);
            if (!c->have_slot[slot]) return fail(WFA_E_STATE, "group %d: plan slot %d holds no plan (wfa_sg_plan_store)", g, slot);
        } else if (groups[g].source == WFA_SRC_F32) {
            if (!c->have_f32)
                return fail(WFA_E_STATE, "group %d: wave_pool_filtered (float32) not resident (wfa_sosfiltfilt_group first)", g);
        } else {
            return fail(WFA_E_INVALID, "group %d: source must be WFA_SRC_SG_FUSED or WFA_SRC_F32, got %d", g, groups[g].source);
        }
    }
    if (c->R > 0 && !group_of_record) return fail(WFA_E_INVALID, "group_of_record is null");
    bool unowned = false;
    for (int64_t r = 0; r < c->R; ++r) {
        const int32_t v = group_of_record[r];
        if (v < -1 || v >= n_groups)
            return fail(WFA_E_INVALID, "group_of_record[%lld] = %d is outside [-1, %d)", (long long)r, v, n_groups);
        unowned |= v < 0;
    }
    if (bl_end > bl_start && bl_start < 0) return fail(WFA_E_INVALID, "baseline window start must be >= 0");
    if (le < 0) le = 0;
    if (re < 0) re = 0;
    if (max_len <= 0) max_len = c->max_len;
    if (max_len < c->max_len)
        return fail(WFA_E_INVALID, "max_len (%d) < longest uploaded record (%d)", max_len, c->max_len);
    if ((rc = groups_pinned(c))) return rc;
    c->pending = wfa_ctx::kPendNone;  // (a queued pass nobody waited for ends here, like in wfa_hits_enqueue)
    wfa_ctx::GroupsPass& G = c->grp;
    if (G.n_groups != n_groups || memcmp(G.groups, groups, (size_t)n_groups * sizeof(wfa_hit_group)) != 0)
        for (int64_t& v : G.last) v = -1;  // other groups than last time: their previous counts say nothing
    G.n_groups = n_groups;
    memcpy(G.groups, groups, (size_t)n_groups * sizeof(wfa_hit_group));
    G.bl_start = bl_start; G.bl_end = bl_end;
    G.le = le; G.re = re; G.max_len = max_len;
    G.single = n_groups == 1 && !unowned;
    G.R = c->R;
    c->n_hits = -1;
    c->rows_index = 0;
    if (c->R == 0) {
        c->n_hits = 0;
        return WFA_OK;
    }
    if (!G.single) {
        if ((rc = c->grp_gor.ensure((size_t)c->R * sizeof(int32_t)))) return rc;
        if ((rc = h2d_copy(c, c->grp_gor.ptr, group_of_record, (size_t)c->R * sizeof(int32_t)))) return rc;
    }
    return groups_run(c, false);
}

int wfa_hits_pending(wfa_ctx* c, int* pending) {
    if (!c || !pending) return fail(WFA_E_INVALID, "null argument");
    *pending = c->pending ? 1 : 0;
    return WFA_OK;
}

int wfa_find_peaks_count(wfa_ctx* c, int source, int signal_mode, int use_derivative, double height, int has_threshold,
                         double threshold, int32_t distance, double prominence, double width, int height_method,
                         int32_t ext, int64_t* n_peaks) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, source))) return rc;
    if (source == WFA_SRC_SG_FUSED) return fail(WFA_E_INVALID, "find_peaks reads wave_pool or a materialised wave_pool_filtered");
    if (!n_peaks) return fail(WFA_E_INVALID, "n_peaks is null");
    if (distance < 1) return fail(WFA_E_INVALID, "`distance` must be greater or equal to 1");  // scipy's message
    if (height_method != WFA_HEIGHT_MINMAX && height_method != WFA_HEIGHT_DIFF)
        return fail(WFA_E_INVALID, "height_method must be WFA_HEIGHT_MINMAX or WFA_HEIGHT_DIFF");
    if (signal_mode < WFA_PEAK_SIGNAL_RECORDS || signal_mode > WFA_PEAK_SIGNAL_ROWS_F64)
        return fail(WFA_E_INVALID, "signal_mode must be WFA_PEAK_SIGNAL_RECORDS, _ROWS or _ROWS_F64");
    c->n_peaks = c->n_chain = -1;
    if (c->R == 0) { c->n_peaks = 0; c->peak_mode = signal_mode; c->peak_gen = c->records_gen; *n_peaks = 0; return WFA_OK; }
    if (c->rows_index == 2) c->rows_index = 0;  // rec_nhits / rec_out_start are this pass's from here on
    const int64_t R = c->R;
    if ((rc = c->rec_nhits.ensure(R * sizeof(int32_t)))) return rc;
    if ((rc = c->rec_out_start.ensure(R * sizeof(int64_t)))) return rc;
    const int64_t nb = scan_blocks_for(R);
    if ((rc = c->scan_blocks.ensure((nb + 1) * sizeof(int64_t)))) return rc;
    if ((rc = c->cursor.ensure(sizeof(unsigned long long)))) return rc;
    WFA_HIP_CHECK(hipMemsetAsync(c->cursor.ptr, 0, sizeof(unsigned long long), c->stream));
    PeakParams pp{};
    pp.use_derivative = use_derivative ? 1 : 0; pp.hmin = height; pp.has_threshold = has_threshold ? 1 : 0;
    pp.tmin = threshold; pp.distance = distance; pp.pmin = prominence; pp.wmin = width;
    pp.ext = ext > 0 ? ext : 0; pp.height_diff = height_method == WFA_HEIGHT_DIFF;
    pp.rows = signal_mode;
    const PoolView pv = pool_view(c);
    const RecView rv = rec_view(c);
    int* err = reinterpret_cast<int*>(c->cursor.ptr);
    int32_t* counts = c->rec_nhits.as<int32_t>();
    auto scan_total = [&](int64_t* starts, int64_t* total) -> int {
        WFA_HIP_CHECK(launch_scan(c->stream, counts, R, c->scan_blocks.as<int64_t>(), starts));
        WFA_HIP_CHECK(hipMemcpyAsync(total, c->scan_blocks.as<int64_t>() + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
        WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        return WFA_OK;
    };
    int64_t total = 0;
    {
        if ((rc = c->rec_tmp_start.ensure(R * sizeof(int64_t)))) return rc;
        if ((rc = c->peak_cand_n.ensure(R * sizeof(int32_t)))) return rc;
        int64_t* cand_start = c->rec_tmp_start.as<int64_t>();
        int32_t* cand_n = c->peak_cand_n.as<int32_t>();
        int64_t n_cand = 0;
        // one walk: counts + the first kPeakSlots candidates of every record in per-record slots (launch_find_peaks_slots);
        // `no_peak_slots` keeps the count + fill pair (two walks, any number of candidates)
        const int K = kPeakSlots;
        const bool slots = !c->opt.no_peak_slots;
        int* overflow = err + 1;
        if (slots) {
            if ((rc = c->peak_slot_pos.ensure((size_t)R * K * sizeof(int32_t)))) return rc;
            if ((rc = c->peak_slot_val.ensure((size_t)R * K * sizeof(double)))) return rc;
            LaunchTimer t(c);
            hipError_t herr = hipSuccess;
            // uniform records: the walk on LDS-staged groups (coalesced); any other layout: one lane per record
            // uniform records: LDS-staged groups (coalesced) -- the plateau machine only on the chunks that can hold a value
            // >= `height` (k_find_peaks_hot), or over every sample (k_find_peaks_staged)
            const bool hot = c->layout.span && !c->opt.no_span && !c->opt.no_peak_hot &&
                             launch_find_peaks_hot(c->stream, source, pv, rv, pp, c->layout.off0, c->layout.L, K, counts,
                                                   c->peak_slot_pos.as<int32_t>(), c->peak_slot_val.as<double>(), overflow, &herr);
            WFA_HIP_CHECK(herr);
            const bool staged = !hot && c->layout.span && !c->opt.no_span &&
                                launch_find_peaks_staged(c->stream, source, pv, rv, pp, c->layout.off0, c->layout.L, K, counts,
                                                         c->peak_slot_pos.as<int32_t>(), c->peak_slot_val.as<double>(), overflow, &herr);
            WFA_HIP_CHECK(herr);
            if (!staged && !hot)
                WFA_HIP_CHECK(launch_find_peaks_slots(c->stream, source, pv, rv, pp, K, counts, c->peak_slot_pos.as<int32_t>(),
                                                      c->peak_slot_val.as<double>(), overflow));
            if ((rc = t.end(hot ? "k_find_peaks_hot" : staged ? "k_find_peaks_staged" : "k_find_peaks_slots"))) return rc;
        } else {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_find_peaks(c->stream, source, false, pv, rv, pp, counts, nullptr, nullptr, nullptr, nullptr));
            if ((rc = t.end("k_find_peaks<count candidates>"))) return rc;
        }
        int over = 0;
        WFA_HIP_CHECK(hipMemcpyAsync(&over, overflow, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if ((rc = scan_total(cand_start, &n_cand))) return rc;
        const size_t nc = (size_t)(n_cand > 0 ? n_cand : 1);
        if ((rc = c->peak_cand_pos.ensure(nc * sizeof(int32_t)))) return rc;
        if ((rc = c->peak_cand_val.ensure(nc * sizeof(double)))) return rc;
        if ((rc = c->peak_cand_rec.ensure(nc * sizeof(int64_t)))) return rc;
        if ((rc = c->peak_cand_state.ensure(nc))) return rc;
        if ((rc = c->peak_accept.ensure(nc * sizeof(int32_t)))) return rc;
        if ((rc = c->peak_ips.ensure(nc * 2 * sizeof(double)))) return rc;
        if ((rc = c->peak_row_start.ensure(nc * sizeof(int64_t)))) return rc;
        int32_t* cpos = c->peak_cand_pos.as<int32_t>();
        double* cval = c->peak_cand_val.as<double>();
        int64_t* crec = c->peak_cand_rec.as<int64_t>();
        uint8_t* cstate = distance > 2 ? c->peak_cand_state.as<uint8_t>() : nullptr;
        int32_t* accept = c->peak_accept.as<int32_t>();
        if (slots && !over) {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_peak_compact(c->stream, R, K, counts, cand_start, c->peak_slot_pos.as<int32_t>(),
                                              c->peak_slot_val.as<double>(), cpos, cval, crec));
            if ((rc = t.end("k_peak_compact"))) return rc;
        } else {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_find_peaks(c->stream, source, true, pv, rv, pp, nullptr, cand_start, cpos, cval, crec));
            if ((rc = t.end("k_find_peaks<fill candidates>"))) return rc;
        }
        if (distance > 2) {  // local maxima are at least 2 samples apart: scipy's distance step keeps all of them otherwise
            WFA_HIP_CHECK(hipMemcpyAsync(cand_n, counts, R * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_peak_select(c->stream, R, cand_n, cand_start, cpos, cval, cstate, distance));
            if ((rc = t.end("k_peak_select"))) return rc;
        }
        {
            LaunchTimer t(c);
            WFA_HIP_CHECK(launch_peak_eval(c->stream, source, pv, rv, pp, n_cand, crec, cpos, cstate, accept, c->peak_ips.as<double>()));
            if ((rc = t.end("k_peak_eval"))) return rc;
        }
        if (n_cand > 0) {
            const int64_t nbc = scan_blocks_for(n_cand);
            if ((rc = c->scan_blocks.ensure((nbc + 1) * sizeof(int64_t)))) return rc;
            WFA_HIP_CHECK(launch_scan(c->stream, accept, n_cand, c->scan_blocks.as<int64_t>(), c->peak_row_start.as<int64_t>()));
            WFA_HIP_CHECK(hipMemcpyAsync(&total, c->scan_blocks.as<int64_t>() + nbc, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
            WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
        }
        if ((rc = c->peak_out.ensure((size_t)total * 48))) return rc;
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_peak_rows(c->stream, source, pv, rv, pp, n_cand, crec, cpos, accept, c->peak_row_start.as<int64_t>(),
                                       c->peak_ips.as<double>(), c->peak_out.as<uint8_t>(), err));
        if ((rc = t.end("k_peak_rows"))) return rc;
    }
    int flag = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&flag, err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (flag)  // numpy's message for np.max of the empty height window (peak_finding.py:606)
        return fail(WFA_E_INVALID, "zero-size array to reduction operation maximum which has no identity");
    // peak_out holds the rows from here on: peak_accept and peak_row_start (like the other per-candidate buffers) have
    // been read for the last time, and wfa_peak_chain_count takes them for its keep flags and their scan
    c->n_peaks = total;
    c->peak_mode = signal_mode;
    c->peak_gen = c->records_gen;
    *n_peaks = total;
    return WFA_OK;
}

int wfa_find_peaks_fill(wfa_ctx* c, void* out_rows, int64_t n_peaks) {
    int rc = use_device(c);
    if (rc) return rc;
    if (c->n_peaks < 0) return fail(WFA_E_STATE, "no find_peaks pass has been run");
    if (n_peaks != c->n_peaks)
        return fail(WFA_E_INVALID, "caller expects %lld rows, the pass produced %lld", (long long)n_peaks, (long long)c->n_peaks);
    if (n_peaks == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->peak_out.ptr, (size_t)n_peaks * 48, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_basic_features(wfa_ctx* c, int source, int64_t h0, int64_t h1, int h_has_end, int64_t a0,
                       int64_t a1, int a_has_end, const double* fixed_baseline, void* out_rows) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, source))) return rc;
    if (source == WFA_SRC_SG_FUSED)
        return fail(WFA_E_INVALID, "basic_features reads wave_pool or a materialised wave_pool_filtered");
    if (c->R == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    FeatParams fp{};
    fp.h0 = h0; fp.h1 = h1; fp.h_has_end = h_has_end;
    fp.a0 = a0; fp.a1 = a1; fp.a_has_end = a_has_end;
    fp.fixed_bl = nullptr;
    if (fixed_baseline) {
        if ((rc = h2d(c, c->fixed_bl, fixed_baseline, (size_t)c->R * sizeof(double)))) return rc;
        fp.fixed_bl = c->fixed_bl.as<double>();
    }
    if ((rc = c->out_rows.ensure((size_t)c->R * 36))) return rc;
    {
        LaunchTimer t(c);
        hipError_t e = hipSuccess;
        if (source == WFA_SRC_RAW && launch_basic_features_wave(c, rec_view(c), fp, c->out_rows.as<uint8_t>(), &e)) {
            WFA_HIP_CHECK(e);
            if ((rc = t.end("k_basic_features_leaf"))) return rc;
        } else {
            WFA_HIP_CHECK(launch_basic_features(c->stream, source, pool_view(c), rec_view(c), sg_params(ctx_plan(c)), fp,
                                                c->out_rows.as<uint8_t>()));
            if ((rc = t.end("k_basic_features"))) return rc;
        }
    }
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->out_rows.ptr, (size_t)c->R * 36, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_find_hits_count(wfa_ctx* c, int source, int64_t n_rows, int32_t row_length, const double* baselines,
                        double threshold, int64_t* n_hits) {
    int rc = use_device(c);
    if (rc) return rc;
    if (source != WFA_SRC_RAW && source != WFA_SRC_F32)
        return fail(WFA_E_INVALID, "find_hits reads dense rows: source must be WFA_SRC_RAW or WFA_SRC_F32");
    if (source == WFA_SRC_RAW ? !c->have_u16 : !c->have_f32) return fail(WFA_E_STATE, "no wave matrix uploaded for this source");
    if (n_rows < 0 || row_length < 0 || !n_hits) return fail(WFA_E_INVALID, "bad arguments");
    if (n_rows * (int64_t)row_length > c->pool_n)
        return fail(WFA_E_INVALID, "wave matrix %lld x %d exceeds the resident pool (%lld samples)", (long long)n_rows,
                    row_length, (long long)c->pool_n);
    c->n_legacy = -1;
    if (n_rows == 0 || row_length == 0) { c->n_legacy = 0; *n_hits = 0; return WFA_OK; }
    if (c->rows_index == 2) c->rows_index = 0;  // rec_nhits / rec_out_start are this pass's from here on
    if (!baselines) return fail(WFA_E_INVALID, "baselines is null");
    if ((rc = c->fixed_bl.ensure((size_t)n_rows * sizeof(double)))) return rc;
    WFA_HIP_CHECK(hipMemcpyAsync(c->fixed_bl.ptr, baselines, (size_t)n_rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = c->rec_nhits.ensure(n_rows * sizeof(int32_t)))) return rc;
    if ((rc = c->rec_out_start.ensure(n_rows * sizeof(int64_t)))) return rc;
    const int64_t nb = scan_blocks_for(n_rows);
    if ((rc = c->scan_blocks.ensure((nb + 1) * sizeof(int64_t)))) return rc;
    const PoolView pv = pool_view(c);
    LaunchTimer t(c);
    WFA_HIP_CHECK(launch_find_hits_legacy(c->stream, source, false, pv, n_rows, row_length, c->fixed_bl.as<double>(), threshold,
                                          c->rec_nhits.as<int32_t>(), nullptr, nullptr, nullptr));
    WFA_HIP_CHECK(launch_scan(c->stream, c->rec_nhits.as<int32_t>(), n_rows, c->scan_blocks.as<int64_t>(),
                              c->rec_out_start.as<int64_t>()));
    int64_t total = 0;
    WFA_HIP_CHECK(hipMemcpyAsync(&total, c->scan_blocks.as<int64_t>() + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if ((rc = c->peak_row_start.ensure((size_t)(total > 0 ? total : 1) * sizeof(int64_t)))) return rc;
    if ((rc = c->peak_ips.ensure((size_t)(total > 0 ? total : 1) * sizeof(int64_t)))) return rc;
    WFA_HIP_CHECK(launch_find_hits_legacy(c->stream, source, true, pv, n_rows, row_length, c->fixed_bl.as<double>(), threshold,
                                          nullptr, c->rec_out_start.as<int64_t>(), c->peak_row_start.as<int64_t>(),
                                          c->peak_ips.as<int64_t>()));
    if ((rc = t.end("k_find_hits_legacy (count + scan + fill)"))) return rc;
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    c->n_legacy = total;
    *n_hits = total;
    return WFA_OK;
}

int wfa_find_hits_fill(wfa_ctx* c, int64_t n_hits, int64_t* event_index, int64_t* start_sample) {
    int rc = use_device(c);
    if (rc) return rc;
    if (c->n_legacy < 0) return fail(WFA_E_STATE, "no find_hits pass has been run");
    if (n_hits != c->n_legacy)
        return fail(WFA_E_INVALID, "caller expects %lld hits, the pass produced %lld", (long long)n_hits, (long long)c->n_legacy);
    if (n_hits == 0) return WFA_OK;
    if (!event_index || !start_sample) return fail(WFA_E_INVALID, "null output");
    WFA_HIP_CHECK(hipMemcpyAsync(event_index, c->peak_row_start.ptr, (size_t)n_hits * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(start_sample, c->peak_ips.ptr, (size_t)n_hits * 8, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

}  // extern "C"

// K10 on either addressing: the per-hit columns up, one launch (enqueued by `launch(position, index, rows, valid)` on
// the context's stream, timed under `name`), rows and valid bytes down.
template <class Launch>
static int width_pass(wfa_ctx* c, int64_t n_hits, const int64_t* position, const int64_t* index, double sampling_rate,
                      const char* name, void* out_rows, uint8_t* valid, Launch launch) {
    if (n_hits == 0) return WFA_OK;
    if (!position || !index || !out_rows || !valid) return fail(WFA_E_INVALID, "null argument");
    if (!(sampling_rate == sampling_rate) || sampling_rate == 0.0) return fail(WFA_E_INVALID, "float division by zero");
    int rc;
    // scratch: positions, row indices, rows, valid bytes
    const size_t b_idx = (size_t)n_hits * sizeof(int64_t);
    if ((rc = c->wh_pos.ensure(b_idx))) return rc;
    if ((rc = c->wh_row.ensure(b_idx))) return rc;
    if ((rc = c->out_rows.ensure((size_t)n_hits * 56))) return rc;
    if ((rc = c->wh_valid.ensure((size_t)n_hits))) return rc;
    WFA_HIP_CHECK(hipMemcpyAsync(c->wh_pos.ptr, position, b_idx, hipMemcpyHostToDevice, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(c->wh_row.ptr, index, b_idx, hipMemcpyHostToDevice, c->stream));
    {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch(c->wh_pos.as<int64_t>(), c->wh_row.as<int64_t>(), c->out_rows.as<uint8_t>(),
                             c->wh_valid.as<uint8_t>()));
        if ((rc = t.end(name))) return rc;
    }
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->out_rows.ptr, (size_t)n_hits * 56, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipMemcpyAsync(valid, c->wh_valid.ptr, (size_t)n_hits, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

extern "C" {

int wfa_waveform_width(wfa_ctx* c, int source, int64_t n_hits, const int64_t* position, const int64_t* row_index,
                       int64_t n_rows, int32_t row_length, double rise_low, double rise_high, double fall_high,
                       double fall_low, double sampling_rate, int interpolation, void* out_rows, uint8_t* valid) {
    int rc = use_device(c);
    if (rc) return rc;
    if (source != WFA_SRC_RAW && source != WFA_SRC_F32)
        return fail(WFA_E_INVALID, "waveform_width reads dense rows: source must be WFA_SRC_RAW or WFA_SRC_F32");
    if (source == WFA_SRC_RAW ? !c->have_u16 : !c->have_f32) return fail(WFA_E_STATE, "no wave matrix uploaded for this source");
    if (n_hits < 0 || n_rows < 0 || row_length < 0) return fail(WFA_E_INVALID, "negative size");
    if (n_rows * (int64_t)row_length > c->pool_n)
        return fail(WFA_E_INVALID, "wave matrix %lld x %d exceeds the resident pool (%lld samples)", (long long)n_rows,
                    row_length, (long long)c->pool_n);
    return width_pass(c, n_hits, position, row_index, sampling_rate, "k_waveform_width", out_rows, valid,
                      [&](const int64_t* d_pos, const int64_t* d_row, uint8_t* d_out, uint8_t* d_valid) {
                          return launch_waveform_width(c->stream, source, pool_view(c), n_hits, d_pos, d_row, n_rows,
                                                       row_length, rise_low, rise_high, fall_high, fall_low,
                                                       sampling_rate, interpolation, d_out, d_valid);
                      });
}

int wfa_waveform_width_records(wfa_ctx* c, int source, int64_t n_hits, const int64_t* position,
                               const int64_t* record_index, double rise_low, double rise_high, double fall_high,
                               double fall_low, double sampling_rate, int interpolation, void* out_rows, uint8_t* valid) {
    int rc = use_device(c);
    if (rc) return rc;
    if (source != WFA_SRC_RAW && source != WFA_SRC_F32)
        return fail(WFA_E_INVALID, "waveform_width reads stored samples: source must be WFA_SRC_RAW or WFA_SRC_F32");
    if ((rc = need_source(c, source))) return rc;  // records (their slices were checked against the pool) + this pool
    if (n_hits < 0) return fail(WFA_E_INVALID, "negative size");
    return width_pass(c, n_hits, position, record_index, sampling_rate, "k_waveform_width_rec", out_rows, valid,
                      [&](const int64_t* d_pos, const int64_t* d_row, uint8_t* d_out, uint8_t* d_valid) {
                          return launch_waveform_width_records(c->stream, source, pool_view(c), rec_view(c), n_hits, d_pos,
                                                               d_row, rise_low, rise_high, fall_high, fall_low,
                                                               sampling_rate, interpolation, d_out, d_valid);
                      });
}

int wfa_peak_chain_count(wfa_ctx* c, int width_source, int feature_source, double rise_low, double rise_high,
                         double fall_high, double fall_low, double sampling_rate, int interpolation, int64_t h0,
                         int64_t h1, int h_has_end, int64_t a0, int64_t a1, int a_has_end, int width_in_samples,
                         const double* class_ranges, uint32_t range_bounds, int conflict_policy, int64_t record_id_base,
                         int64_t* n_rows) {
    return wfa_peak_chain_count_fixed(c, width_source, feature_source, rise_low, rise_high, fall_high, fall_low,
                                      sampling_rate, interpolation, h0, h1, h_has_end, a0, a1, a_has_end, width_in_samples,
                                      class_ranges, range_bounds, conflict_policy, record_id_base, nullptr, n_rows);
}

int wfa_peak_chain_count_fixed(wfa_ctx* c, int width_source, int feature_source, double rise_low, double rise_high,
                               double fall_high, double fall_low, double sampling_rate, int interpolation, int64_t h0,
                               int64_t h1, int h_has_end, int64_t a0, int64_t a1, int a_has_end, int width_in_samples,
                               const double* class_ranges, uint32_t range_bounds, int conflict_policy,
                               int64_t record_id_base, const double* fixed_baseline, int64_t* n_rows) {
    int rc = use_device(c);
    if (rc) return rc;
    if (!n_rows) return fail(WFA_E_INVALID, "n_rows is null");
    if ((width_source != WFA_SRC_RAW && width_source != WFA_SRC_F32) ||
        (feature_source != WFA_SRC_RAW && feature_source != WFA_SRC_F32))
        return fail(WFA_E_INVALID, "peak_chain reads stored samples: sources must be WFA_SRC_RAW or WFA_SRC_F32");
    if (range_bounds >> 12) return fail(WFA_E_INVALID, "range_bounds has bits above the six ranges");
    if (conflict_policy < WFA_S1S2_UNKNOWN || conflict_policy > WFA_S1S2_PREFER_S2)
        return fail(WFA_E_INVALID, "conflict_policy must be WFA_S1S2_UNKNOWN, _PREFER_S1 or _PREFER_S2");
    if (range_bounds && !class_ranges) return fail(WFA_E_INVALID, "class_ranges is null");
    c->n_chain = -1;
    if (c->n_peaks < 0) return fail(WFA_E_STATE, "no find_peaks pass has been run");
    if (c->peak_mode != WFA_PEAK_SIGNAL_RECORDS)
        return fail(WFA_E_STATE, "peak_chain needs the rows of a WFA_PEAK_SIGNAL_RECORDS find_peaks pass");
    if (c->peak_gen != c->records_gen)
        return fail(WFA_E_STATE, "the records have been replaced since the find_peaks pass: run it again");
    if ((rc = need_source(c, width_source))) return rc;  // records (their slices were checked against the pool) + the pools
    if ((rc = need_source(c, feature_source))) return rc;
    const int64_t n = c->n_peaks;
    if (n == 0) { c->n_chain = 0; *n_rows = 0; return WFA_OK; }
    if (!(sampling_rate == sampling_rate) || sampling_rate == 0.0) return fail(WFA_E_INVALID, "float division by zero");
    // scratch: feature rows, row slots, kept rows; keep flags and their scan in find_peaks' per-candidate buffers (the
    // pass has read them for the last time: its rows are in peak_out)
    if ((rc = c->pc_feat.ensure((size_t)c->R * 36))) return rc;
    if ((rc = c->pc_rows.ensure((size_t)n * 45))) return rc;
    if ((rc = c->peak_accept.ensure((size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = c->peak_row_start.ensure((size_t)n * sizeof(int64_t)))) return rc;
    const int64_t nb = scan_blocks_for(n);
    if ((rc = c->scan_blocks.ensure((nb + 1) * sizeof(int64_t)))) return rc;
    FeatParams fp{};
    fp.h0 = h0; fp.h1 = h1; fp.h_has_end = h_has_end;
    fp.a0 = a0; fp.a1 = a1; fp.a_has_end = a_has_end;
    fp.fixed_bl = nullptr;
    if (fixed_baseline) {  // per record, NaN = none: the column of wfa_basic_features
        if ((rc = h2d(c, c->fixed_bl, fixed_baseline, (size_t)c->R * sizeof(double)))) return rc;
        fp.fixed_bl = c->fixed_bl.as<double>();
    }
    {
        LaunchTimer t(c);
        hipError_t e = hipSuccess;
        if (feature_source == WFA_SRC_RAW && launch_basic_features_wave(c, rec_view(c), fp, c->pc_feat.as<uint8_t>(), &e)) {
            WFA_HIP_CHECK(e);
            if ((rc = t.end("k_basic_features_leaf"))) return rc;
        } else {
            WFA_HIP_CHECK(launch_basic_features(c->stream, feature_source, pool_view(c), rec_view(c), sg_params(ctx_plan(c)), fp,
                                                c->pc_feat.as<uint8_t>()));
            if ((rc = t.end("k_basic_features"))) return rc;
        }
    }
    ChainParams cp{};
    for (int k = 0; k < 6; ++k) {
        cp.lo[k] = (range_bounds >> (2 * k)) & 1u ? class_ranges[2 * k] : 0.0;
        cp.hi[k] = (range_bounds >> (2 * k)) & 2u ? class_ranges[2 * k + 1] : 0.0;
    }
    cp.bounds = range_bounds;
    cp.width_in_samples = width_in_samples ? 1 : 0;
    cp.policy = conflict_policy;
    cp.record_id_base = record_id_base;
    int32_t* keep = c->peak_accept.as<int32_t>();
    int64_t* start = c->peak_row_start.as<int64_t>();
    {
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_peak_chain(c->stream, width_source, pool_view(c), rec_view(c), n, c->peak_out.as<uint8_t>(),
                                        c->pc_feat.as<uint8_t>(), rise_low, rise_high, fall_high, fall_low, sampling_rate,
                                        interpolation, cp, c->pc_rows.as<uint8_t>(), keep));
        if ((rc = t.end("k_peak_chain"))) return rc;
    }
    int64_t kept = 0;
    WFA_HIP_CHECK(launch_scan(c->stream, keep, n, c->scan_blocks.as<int64_t>(), start));
    WFA_HIP_CHECK(hipMemcpyAsync(&kept, c->scan_blocks.as<int64_t>() + nb, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    if (kept < 0 || kept > n) return fail(WFA_E_HIP, "peak_chain kept %lld of %lld rows", (long long)kept, (long long)n);
    if (kept > 0) {
        if ((rc = c->pc_out.ensure((size_t)kept * 45))) return rc;
        LaunchTimer t(c);
        WFA_HIP_CHECK(launch_peak_chain_compact(c->stream, n, c->pc_rows.as<uint8_t>(), keep, start, c->pc_out.as<uint8_t>()));
        if ((rc = t.end("k_peak_chain_compact"))) return rc;
    }
    c->n_chain = kept;
    *n_rows = kept;
    return WFA_OK;
}

int wfa_peak_chain_fill(wfa_ctx* c, void* out_rows, int64_t n_rows) {
    int rc = use_device(c);
    if (rc) return rc;
    if (c->n_chain < 0) return fail(WFA_E_STATE, "no peak_chain pass has been run");
    if (n_rows != c->n_chain)
        return fail(WFA_E_INVALID, "caller expects %lld rows, the pass produced %lld", (long long)n_rows, (long long)c->n_chain);
    if (n_rows == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->pc_out.ptr, (size_t)n_rows * 45, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_width_integral(wfa_ctx* c, int source, double q_low, double q_high, double dt, void* out_rows) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, source))) return rc;
    if (source == WFA_SRC_SG_FUSED)
        return fail(WFA_E_INVALID, "width_integral reads wave_pool or a materialised wave_pool_filtered");
    if (!(q_low > 0.0) || !(q_high < 1.0) || !(q_low < q_high))  // waveform_width_integral.py:95-96
        return fail(WFA_E_INVALID, "q_low/q_high invalid: q_low=%g, q_high=%g", q_low, q_high);
    if (c->R == 0) return WFA_OK;
    if (!out_rows) return fail(WFA_E_INVALID, "out_rows is null");
    WidthParams wp{q_low, q_high, dt};
    int rc2 = c->out_rows.ensure((size_t)c->R * 52);
    if (rc2) return rc2;
    {
        LaunchTimer t(c);
        hipError_t e = hipSuccess;
        if (source == WFA_SRC_RAW && launch_width_integral_wave(c, rec_view(c), wp, c->out_rows.as<uint8_t>(), &e)) {
            WFA_HIP_CHECK(e);
            if ((rc = t.end("k_width_integral_leaf"))) return rc;
        } else {
            WFA_HIP_CHECK(launch_width_integral(c->stream, source, pool_view(c), rec_view(c), sg_params(ctx_plan(c)), wp,
                                                c->out_rows.as<uint8_t>()));
            if ((rc = t.end("k_width_integral"))) return rc;
        }
    }
    WFA_HIP_CHECK(hipMemcpyAsync(out_rows, c->out_rows.ptr, (size_t)c->R * 52, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_features_both(wfa_ctx* c, int64_t h0, int64_t h1, int h_has_end, int64_t a0, int64_t a1, int a_has_end,
                      double q_low, double q_high, double dt, void* out_basic, void* out_width) {
    int rc = use_device(c);
    if (rc) return rc;
    if ((rc = need_source(c, WFA_SRC_RAW))) return rc;
    if (!(q_low > 0.0) || !(q_high < 1.0) || !(q_low < q_high))  // waveform_width_integral.py:95-96
        return fail(WFA_E_INVALID, "q_low/q_high invalid: q_low=%g, q_high=%g", q_low, q_high);
    if (c->R == 0) return WFA_OK;
    FeatParams fp{};
    fp.h0 = h0; fp.h1 = h1; fp.h_has_end = h_has_end;
    fp.a0 = a0; fp.a1 = a1; fp.a_has_end = a_has_end;
    fp.fixed_bl = nullptr;
    WidthParams wp{q_low, q_high, dt};
    if ((rc = c->out_rows.ensure((size_t)c->R * 36)) || (rc = c->out_rows2.ensure((size_t)c->R * 52))) return rc;
    uint8_t* ob = c->out_rows.as<uint8_t>();
    uint8_t* ow = c->out_rows2.as<uint8_t>();
    {
        LaunchTimer t(c);
        hipError_t e = hipSuccess;
        if (launch_features_both_wave(c, rec_view(c), fp, wp, ob, ow, &e)) {
            WFA_HIP_CHECK(e);
            if ((rc = t.end("k_features_both_leaf"))) return rc;
        } else {  // layout or ranges outside the fused kernel: the two kernels, one after the other
            if (launch_basic_features_wave(c, rec_view(c), fp, ob, &e)) {
                WFA_HIP_CHECK(e);
                if ((rc = t.end("k_basic_features_leaf"))) return rc;
            } else {
                WFA_HIP_CHECK(launch_basic_features(c->stream, WFA_SRC_RAW, pool_view(c), rec_view(c), sg_params(ctx_plan(c)), fp, ob));
                if ((rc = t.end("k_basic_features"))) return rc;
            }
            LaunchTimer t2(c);
            if (launch_width_integral_wave(c, rec_view(c), wp, ow, &e)) {
                WFA_HIP_CHECK(e);
                if ((rc = t2.end("k_width_integral_leaf"))) return rc;
            } else {
                WFA_HIP_CHECK(launch_width_integral(c->stream, WFA_SRC_RAW, pool_view(c), rec_view(c), sg_params(ctx_plan(c)), wp, ow));
                if ((rc = t2.end("k_width_integral"))) return rc;
            }
        }
    }
    if (out_basic) WFA_HIP_CHECK(hipMemcpyAsync(out_basic, ob, (size_t)c->R * 36, hipMemcpyDeviceToHost, c->stream));
    if (out_width) WFA_HIP_CHECK(hipMemcpyAsync(out_width, ow, (size_t)c->R * 52, hipMemcpyDeviceToHost, c->stream));
    WFA_HIP_CHECK(hipStreamSynchronize(c->stream));
    return WFA_OK;
}

int wfa_profile_enable(wfa_ctx* c, int on) {
    if (!c) return fail(WFA_E_INVALID, "null context");
    if (!on) (void)profile_flush(c);
    c->prof_on = on != 0;
    c->prof_level = on == 2 ? 2 : (on ? 1 : 0);
    return WFA_OK;
}

int wfa_profile_reset(wfa_ctx* c) {
    if (!c) return fail(WFA_E_INVALID, "null context");
    (void)profile_flush(c);
    c->prof.clear();
    return WFA_OK;
}

int wfa_profile_get(wfa_ctx* c, int idx, char* name, size_t name_len, double* total_ms, int64_t* launches) {
    if (!c) return fail(WFA_E_INVALID, "null context");
    (void)hipSetDevice(c->device);
    (void)profile_flush(c);
    if (idx < 0 || idx >= (int)c->prof.size()) return WFA_E_INVALID;
    const ProfEntry& e = c->prof[idx];
    if (name && name_len) snprintf(name, name_len, "%s", e.name.c_str());
    if (total_ms) *total_ms = e.total_ms;
    if (launches) *launches = e.launches;
    return WFA_OK;
}

}  // extern "C"
