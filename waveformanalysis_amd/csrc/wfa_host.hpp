// Host-only pieces of libwfa_hip.so as plain C++17 (no HIP): the code here is what the library runs on the CPU side of
// the path, and what `make SANITIZE=1 host_check` builds with AddressSanitizer + UndefinedBehaviorSanitizer behind a
// stand-in for the device (csrc/host_check.cpp; SURVEY section 5: the reference has no sanitizer run of its own).
//   * v1725_index / v1725_index_block: header walk of a CAEN V1725 DAW_DEMO binary stream, whole or block by block
//     (reference utils/formats/v1725.py:66-114);
//   * staged_copy: host -> device through two pinned staging buffers, a few host threads filling one while the other is
//     on the wire (the ring of wfa_upload_pool_u16 / wfa_upload_pool_f32);
//   * records_uniform / uniform_layout: the uniform-record layout of a records upload (both upload routes);
//   * baseline_window: the clamp of a baseline window to the longest uploaded record (wfa_baseline_mean, the hit pass);
//   * dense_load_bytes / dense_rows_per_batch / dense_unpack_lane: load width, batch size and the per-lane body of
//     k_dense_unpack (wfa_upload_dense_rows).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>

#include "wfa_hip.h"

namespace wfa {

// What a records upload found about its layout.  span: every record L samples (a multiple of 8, >= 24), back to back from
// the 16-byte aligned sample off0, one polarity class -- the uniform-record kernels read the pool in place.  pad: uniform
// records over a uint16 pool whose L >= 32 is no multiple of 16 -- the span16 kernels need every lane's 16-sample chunk
// inside one record and read a shadow copy of the pool with the records at stride S = roundup16(L) (S = L without pad).
struct UniformLayout {
    bool span = false, pad = false, positive = false;
    int32_t L = 0, S = 0;
    int64_t off0 = 0;
};

namespace host {

// every record as long as record 0, back to back behind it, in its polarity class (positive or not)
inline bool records_uniform(int64_t R, const int64_t* off, const int32_t* len, const int8_t* pol) {
    for (int64_t r = 0; r < R; ++r)
        if (len[r] != len[0] || off[r] != off[0] + r * (int64_t)len[0] ||
            (pol[r] == WFA_POL_POSITIVE) != (pol[0] == WFA_POL_POSITIVE))
            return false;
    return true;
}

// (len0, off0, pol0: record 0 of R records that are `uniform`)
inline UniformLayout uniform_layout(bool uniform, int64_t R, int32_t len0, int64_t off0, int8_t pol0, bool have_u16) {
    UniformLayout u;
    if (!uniform || R <= 0) return u;
    u.span = len0 >= 24 && len0 % 8 == 0 && off0 % 8 == 0;
    u.pad = have_u16 && len0 >= 32 && len0 % 16 != 0;
    if (!u.span && !u.pad) return u;
    u.positive = pol0 == WFA_POL_POSITIVE;
    u.L = len0;
    u.S = u.pad ? (len0 + 15) / 16 * 16 : len0;
    u.off0 = off0;
    return u;
}

// The baseline window [start, end) as the kernels see it.  Every kernel clamps end to its record's length and takes a
// window that is empty after that as NaN, so min(start, max_len) and min(end, max_len) give the same baselines
// (max_len: the longest uploaded record); a window that is empty for every record becomes (max_len, max_len).  No kernel
// then adds a lane number to a start above max_len <= WFA_MAX_RECORD_SAMPLES.  (Callers refuse start < 0; here it counts
// as empty.)
struct BaselineWindow {
    int32_t start, end;
};
inline BaselineWindow baseline_window(int32_t start, int32_t end, int32_t max_len) {
    if (max_len < 0) max_len = 0;
    const int32_t e = end < max_len ? end : max_len;
    if (start < 0 || e <= start) return {max_len, max_len};
    return {start, e};
}

// Returns 0, or -1 with a message in err (the stream is malformed: a channel block shorter than its own header).
// capacity = rows the output columns hold (0: count only); *n_waves = waves in the stream either way.
// at_file_end: buf ends where the file ends -- a short header or payload ends the stream, the complete waves of the cut
// event count, *consumed_bytes = n_bytes.  Otherwise buf is a window into a longer file: only whole events count,
// *consumed_bytes = where the last whole event ends (0: not even one), and rows behind *n_waves are not meaningful.
inline int v1725_index_block(const uint8_t* buf, int64_t n_bytes, bool at_file_end, int64_t capacity, int16_t* channel,
                             int64_t* timestamp, uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset,
                             int32_t* n_samples, int64_t* n_waves, int64_t* consumed_bytes, char* err, size_t err_len) {
    int64_t pos = 0, k = 0, whole_pos = 0, whole_k = 0;
    bool stop = false;
    while (!stop && n_bytes - pos >= 16) {  // a short event header ends the stream
        const uint8_t* eh = buf + pos;
        pos += 16;
        const unsigned mask = (unsigned)eh[4] | ((unsigned)eh[11] << 8);
        for (int ch = 0; ch < 16 && !stop; ++ch) {
            if (!((mask >> ch) & 1u)) continue;
            if (n_bytes - pos < 12) { pos = n_bytes; stop = true; break; }  // short channel header
            const uint8_t* h = buf + pos;
            pos += 12;
            const int64_t ch_size = ((int64_t)h[0] | ((int64_t)h[1] << 8) | ((int64_t)h[2] << 16)) & 0x3fffff;
            if (ch_size < 3) {
                if (err && err_len)
                    snprintf(err, err_len, "V1725 channel size %lld < 3 words at byte %lld", (long long)ch_size, (long long)(pos - 12));
                return -1;
            }
            const int64_t sig_bytes = (ch_size - 3) << 2;
            if (n_bytes - pos < sig_bytes) { pos = n_bytes; stop = true; break; }  // short waveform
            if (k < capacity) {
                int64_t ts = 0;
                for (int b = 5; b >= 0; --b) ts = (ts << 8) | h[4 + b];
                channel[k] = (int16_t)ch;
                timestamp[k] = ts;
                trunc[k] = (uint8_t)((h[3] >> 6) & 1u);
                baseline[k] = (uint16_t)(h[10] | (h[11] << 8));
                payload_offset[k] = pos;
                n_samples[k] = (int32_t)(sig_bytes >> 1);
            }
            ++k;
            pos += sig_bytes;
        }
        if (!stop) { whole_pos = pos; whole_k = k; }
    }
    *n_waves = at_file_end ? k : whole_k;
    if (consumed_bytes) *consumed_bytes = at_file_end ? n_bytes : whole_pos;
    return 0;
}

// the whole stream in one buffer
inline int v1725_index(const uint8_t* buf, int64_t n_bytes, int64_t capacity, int16_t* channel, int64_t* timestamp,
                       uint8_t* trunc, uint16_t* baseline, int64_t* payload_offset, int32_t* n_samples, int64_t* n_waves,
                       char* err, size_t err_len) {
    return v1725_index_block(buf, n_bytes, true, capacity, channel, timestamp, trunc, baseline, payload_offset, n_samples,
                             n_waves, nullptr, err, err_len);
}

// ---- dense rows (wfa_upload_dense_rows): the batch / alignment arithmetic and the per-lane body of k_dense_unpack ----
// The body is plain C++ shared by the kernel and by host_check, which runs every lane of every batch over exactly-sized
// heap buffers under the sanitizers: an out-of-range or misaligned access of the kernel is one of this function.
#if defined(__HIPCC__)
#define WFA_HD __host__ __device__ __forceinline__
#else
#define WFA_HD inline
#endif

// Widest load (bytes, a power of two <= 16) every row of a (wave_offset, row_bytes) layout allows: the batch buffer is
// 256-byte aligned, so row r's wave starts at r * row_bytes + wave_offset, a multiple of the result, and a load of that
// width aligned inside the buffer never leaves the row (row_bytes is a multiple of it too).  elem_bytes divides both.
inline int dense_load_bytes(int64_t wave_offset, int64_t row_bytes, int elem_bytes) {
    int w = elem_bytes;
    while (w < 16 && wave_offset % (2 * w) == 0 && row_bytes % (2 * w) == 0) w *= 2;
    return w;
}

// Rows per batch: whole rows, at least one, at most batch_bytes and at most 1 GiB of them (the rule of wfa_st_pack and
// wfa_view_gather).
inline int64_t dense_rows_per_batch(int64_t n_rows, int64_t row_bytes, int64_t batch_bytes) {
    const int64_t cap = batch_bytes < 1 ? 1 : (batch_bytes > (1ll << 30) ? (1ll << 30) : batch_bytes);
    const int64_t fit = cap / row_bytes;
    const int64_t rows = fit < 1 ? 1 : fit;
    return rows < n_rows ? rows : n_rows;
}

// One batch of whole rows in its device buffer.  Elements are elem_bytes wide; the pool is the flat row-major matrix.
struct DenseBatch {
    uint64_t out_begin, out_end;  // pool elements [row0 * L, (row0 + rows) * L) this batch writes
    int64_t row0;                 // first row of the batch
    uint32_t L;                   // elements per row (> 0)
    uint32_t row_elems;           // row_bytes / elem_bytes
    uint32_t wave_elem;           // wave_offset / elem_bytes
};

// 16-byte chunks of the pool (absolute, so every full chunk is a 16-byte aligned store) that hold an element of the batch
inline uint64_t dense_first_chunk(const DenseBatch& b, int elem_bytes) { return b.out_begin / (16u / elem_bytes); }
inline uint64_t dense_chunk_count(const DenseBatch& b, int elem_bytes) {
    const uint64_t epl = 16u / elem_bytes;
    return b.out_end > b.out_begin ? (b.out_end + epl - 1) / epl - b.out_begin / epl : 0;
}

struct alignas(16) DenseV16 { uint64_t lo, hi; };

template <int W>
WFA_HD void dense_load_word(const uint8_t* p, uint64_t& q0, uint64_t& q1) {
    if constexpr (W == 2) q0 = *reinterpret_cast<const uint16_t*>(p);
    else if constexpr (W == 4) q0 = *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (W == 8) q0 = *reinterpret_cast<const uint64_t*>(p);
    else { const DenseV16 v = *reinterpret_cast<const DenseV16*>(p); q0 = v.lo; q1 = v.hi; }
}

// The lane that owns pool chunk `chunk` (16 bytes = 16 / ES consecutive elements; the lanes of a wave own consecutive
// chunks, so they read consecutive bytes of a row).  Reads its elements with aligned W-byte loads, each word once, and
// only words that hold an element of the batch; writes one 16-byte vector when the whole chunk belongs to the batch,
// single elements at the batch's two ragged ends.  SIGNED (ES == 2): returns the first row (absolute) among its elements
// with the sign bit set, else -1.
template <int ES, int W, bool SIGNED>
WFA_HD int64_t dense_unpack_lane(const uint8_t* src, uint8_t* pool, const DenseBatch& b, uint64_t chunk) {
    constexpr uint32_t EPL = 16 / ES, WE = W / ES;
    const uint64_t i0 = chunk * EPL;
    const uint64_t first = i0 > b.out_begin ? i0 : b.out_begin;
    const uint64_t last = i0 + EPL < b.out_end ? i0 + EPL : b.out_end;
    if (first >= last) return -1;
    const uint32_t e = (uint32_t)(first - b.out_begin);  // < 2^31 / ES: a batch buffer is shorter than 2 GiB
    uint32_t r = e / b.L, j = e - r * b.L;
    uint32_t a = r * b.row_elems + b.wave_elem + j;      // element address inside the batch buffer
    uint32_t cur = 0xffffffffu;
    uint64_t q0 = 0, q1 = 0;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    int64_t negative = -1;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t t = 0; t < EPL; ++t) {
        const uint64_t i = i0 + t;
        if (i < first || i >= last) continue;
        const uint32_t w = a / WE;
        if (w != cur) {
            dense_load_word<W>(src + (size_t)w * W, q0, q1);
            cur = w;
        }
        const uint32_t bit = (a % WE) * (ES * 8);
        uint64_t q = q0;
        if constexpr (W == 16) q = bit < 64 ? q0 : q1;
        const uint32_t v = (uint32_t)(q >> (bit & 63u)) & (ES == 2 ? 0xffffu : 0xffffffffu);
        if (SIGNED && (v & 0x8000u) && negative < 0) negative = b.row0 + r;
        if constexpr (ES == 2) o[t / 2] |= v << (16 * (t & 1));
        else o[t] = v;
        ++a;
        if (++j == b.L) {
            j = 0;
            ++r;
            a += b.row_elems - b.L;
        }
    }
    uint8_t* dst = pool + i0 * ES;
    if (last - first == EPL) {
        DenseV16 v;
        v.lo = o[0] | ((uint64_t)o[1] << 32);
        v.hi = o[2] | ((uint64_t)o[3] << 32);
        *reinterpret_cast<DenseV16*>(dst) = v;
    } else {
        for (uint32_t t = 0; t < EPL; ++t) {
            const uint64_t i = i0 + t;
            if (i < first || i >= last) continue;
            if constexpr (ES == 2) reinterpret_cast<uint16_t*>(dst)[t] = (uint16_t)(o[t / 2] >> (16 * (t & 1)));
            else reinterpret_cast<uint32_t*>(dst)[t] = o[t];
        }
    }
    return negative;
}

constexpr int kStageThreads = 4;

inline void parallel_memcpy(void* dst, const void* src, size_t bytes, size_t serial_below = (8u << 20)) {
    if (bytes < serial_below) { memcpy(dst, src, bytes); return; }
    std::thread th[kStageThreads - 1];
    const size_t part = (bytes / kStageThreads + 4095) & ~(size_t)4095;
    for (int t = 1; t < kStageThreads; ++t) {
        const size_t o = (size_t)t * part;
        if (o >= bytes) break;
        const size_t n = o + part < bytes ? part : bytes - o;
        th[t - 1] = std::thread([=] { memcpy((char*)dst + o, (const char*)src + o, n); });
    }
    memcpy(dst, src, part < bytes ? part : bytes);
    for (auto& x : th) if (x.joinable()) x.join();
}

// src -> dst in chunks of stage_bytes through stage[0] / stage[1].  `copy(dst, staged, n, b)` queues the device copy out of
// staging buffer b and marks its completion; `wait(b)` blocks until the last copy queued out of buffer b has finished.
// Both return 0 or an error code, which ends the transfer.  The caller waits for the whole queue afterwards.
template <class Copy, class Wait>
inline int staged_copy(void* dst, const void* src, size_t bytes, void* const stage[2], size_t stage_bytes, Copy copy, Wait wait,
                       size_t serial_below = (8u << 20)) {
    bool used[2] = {false, false};
    int b = 0;
    for (size_t off = 0; off < bytes; off += stage_bytes, b ^= 1) {
        const size_t n = bytes - off < stage_bytes ? bytes - off : stage_bytes;
        if (used[b])
            if (int rc = wait(b)) return rc;  // the copy out of this buffer has finished
        parallel_memcpy(stage[b], (const char*)src + off, n, serial_below);
        if (int rc = copy((char*)dst + off, stage[b], n, b)) return rc;
        used[b] = true;
    }
    return 0;
}

}  // namespace host
}  // namespace wfa
