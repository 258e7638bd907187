// Sanitizer driver for the host-only C++ of libwfa_hip.so (wfa_host.hpp), built by `make SANITIZE=1 host_check` with
// -fsanitize=address,undefined and run by tests/test_host_sanitized.py on the CPU box (the pool's GPU boxes offer no
// GPU AddressSanitizer; the reference has no sanitizer run at all: SURVEY section 5).  The device is a stand-in: an
// in-order queue of asynchronous copies executed by one thread, with a completion stamp per staging buffer -- what the
// HIP stream + events are to the real ring.
//   host_check v1725 <blob file>     header walk over the whole stream and over every truncation of it
//   host_check v1725-prefixes <blob file>  the walk over EVERY prefix 0..n of a small stream: wave total and a digest
//   host_check ring <bytes> <stage>  staged copy of a pseudo-random buffer, compared byte for byte
//   host_check layout <cases file>   the uniform-record layout of every records table in the file
//   host_check window <cases file>   the baseline window the kernels see for every (start, end, max_len) in the file
//   host_check dense                 every lane of k_dense_unpack over exactly-sized batch buffers and pools
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <vector>

#include "wfa_host.hpp"

namespace {

struct AsyncQueue {  // one worker, tasks in order (a HIP stream)
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    bool done = false;
    std::thread worker;
    AsyncQueue() : worker([this] { run(); }) {}
    ~AsyncQueue() {
        { std::lock_guard<std::mutex> l(m); done = true; }
        cv.notify_all();
        worker.join();
    }
    void push(std::function<void()> f) {
        { std::lock_guard<std::mutex> l(m); q.push_back(std::move(f)); }
        cv.notify_all();
    }
    void run() {
        for (;;) {
            std::function<void()> f;
            {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [this] { return done || !q.empty(); });
                if (q.empty()) return;
                f = std::move(q.front());
                q.pop_front();
            }
            f();
        }
    }
};

int check_v1725(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> blob;
    uint8_t tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) blob.insert(blob.end(), tmp, tmp + got);
    fclose(f);
    char err[160] = "";
    auto walk = [&](int64_t n_bytes, bool print) {
        // exactly-sized copy of the prefix: a read behind it is a heap-buffer-overflow for the sanitizer
        std::vector<uint8_t> buf(blob.begin(), blob.begin() + n_bytes);
        int64_t n = 0;
        int rc = wfa::host::v1725_index(buf.data(), n_bytes, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, err, sizeof(err));
        if (rc) return (int64_t)-1;
        std::vector<int16_t> ch(n);
        std::vector<int64_t> ts(n), off(n);
        std::vector<uint8_t> tr(n);
        std::vector<uint16_t> bl(n);
        std::vector<int32_t> ns(n);
        int64_t n2 = 0;
        rc = wfa::host::v1725_index(buf.data(), n_bytes, n, ch.data(), ts.data(), tr.data(), bl.data(), off.data(), ns.data(), &n2, err, sizeof(err));
        if (rc || n2 != n) return (int64_t)-2;
        uint64_t d_ts = 0, d_ch = 0, d_bl = 0, samples = 0, d_first = 0;
        for (int64_t k = 0; k < n; ++k) {
            d_ts += (uint64_t)ts[k] * (uint64_t)(k + 1); d_ch += (uint64_t)ch[k]; d_bl += bl[k]; samples += (uint64_t)ns[k];
            if (ns[k] > 0) d_first += (uint64_t)(buf[off[k]] | (buf[off[k] + 1] << 8));  // first sample of every wave: inside the buffer
            if (off[k] + 2 * (int64_t)ns[k] > n_bytes) return (int64_t)-3;
        }
        if (print)
            printf("{\"waves\": %lld, \"samples\": %llu, \"ts_digest\": %llu, \"channel_sum\": %llu, \"baseline_sum\": %llu, \"first_sample_sum\": %llu}\n",
                   (long long)n, (unsigned long long)samples, (unsigned long long)d_ts, (unsigned long long)d_ch,
                   (unsigned long long)d_bl, (unsigned long long)d_first);
        return n;
    };
    const int64_t full = walk((int64_t)blob.size(), true);
    if (full < 0) { fprintf(stderr, "walk failed: %s\n", err); return 1; }
    // every truncation of the first 4 KiB and of the last 4 KiB, and a stride through the middle: never more waves than
    // the whole stream, never a read outside the prefix
    int64_t prev = 0;
    const int64_t n = (int64_t)blob.size();
    for (int64_t cut = 0; cut <= n; cut += (cut < 4096 || cut > n - 4096) ? 1 : 997) {
        const int64_t w = walk(cut, false);
        if (w < 0 || w > full || w < prev) { fprintf(stderr, "truncation at %lld: %lld waves (prev %lld, full %lld)\n", (long long)cut, (long long)w, (long long)prev, (long long)full); return 1; }
        prev = w;
    }
    // a channel block that claims fewer than 3 words is an error with a message, not a crash
    if (blob.size() >= 28) {
        std::vector<uint8_t> bad(blob.begin(), blob.begin() + 28);
        bad[4] |= 1;  // channel 0 present
        bad[16] = 2; bad[17] = 0; bad[18] &= 0xc0;
        int64_t nn = 0;
        if (wfa::host::v1725_index(bad.data(), 28, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &nn, err, sizeof(err)) != -1 ||
            !strstr(err, "< 3 words")) { fprintf(stderr, "malformed block not reported\n"); return 1; }
    }
    return 0;
}

// Every prefix length 0..n of the stream as an exactly-sized heap copy (a read behind it is a heap-buffer-overflow for
// the sanitizer): count pass, fill pass, and one running digest over every column of every wave of every prefix, which
// tests/test_host_sanitized.py recomputes from a plain-Python walk (tests/ingest_edges_util.py prefix_sweep_digest).
int check_v1725_prefixes(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<uint8_t> blob;
    uint8_t tmp[4096];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) blob.insert(blob.end(), tmp, tmp + got);
    fclose(f);
    char err[160] = "";
    uint64_t digest = 0, total = 0;
    for (size_t cut = 0; cut <= blob.size(); ++cut) {
        uint8_t* buf = (uint8_t*)malloc(cut ? cut : 1);  // cut == 0: one byte nobody may read
        if (!buf) return 2;
        if (cut) memcpy(buf, blob.data(), cut);
        int64_t n = 0, n2 = 0;
        int rc = wfa::host::v1725_index(buf, (int64_t)cut, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &n, err, sizeof(err));
        std::vector<int16_t> ch((size_t)n);
        std::vector<int64_t> ts((size_t)n), off((size_t)n);
        std::vector<uint8_t> tr((size_t)n);
        std::vector<uint16_t> bl((size_t)n);
        std::vector<int32_t> ns((size_t)n);
        if (!rc) rc = wfa::host::v1725_index(buf, (int64_t)cut, n, ch.data(), ts.data(), tr.data(), bl.data(), off.data(), ns.data(), &n2, err, sizeof(err));
        free(buf);
        if (rc || n2 != n) { fprintf(stderr, "prefix %zu: walk failed: %s\n", cut, err); return 1; }
        for (int64_t k = 0; k < n; ++k) {
            if (off[k] < 0 || off[k] + 2 * (int64_t)ns[k] > (int64_t)cut) { fprintf(stderr, "prefix %zu: wave %lld outside the prefix\n", cut, (long long)k); return 1; }
            const uint64_t term = (uint64_t)ch[k] + 31ull * (uint64_t)ts[k] + 131ull * tr[k] + 8191ull * bl[k] +
                                  65537ull * (uint64_t)off[k] + 1000033ull * (uint64_t)ns[k];
            digest = digest * 1000003ull + term * (uint64_t)(k + 1);
        }
        total += (uint64_t)n;
    }
    printf("{\"prefixes\": %zu, \"waves\": %llu, \"digest\": %llu}\n", blob.size() + 1, (unsigned long long)total,
           (unsigned long long)digest);
    return 0;
}

int check_ring(size_t bytes, size_t stage_bytes) {
    std::vector<uint8_t> src(bytes), dst(bytes, 0);
    uint64_t s = 88172645463325252ull;
    for (size_t i = 0; i < bytes; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; src[i] = (uint8_t)s; }
    std::vector<uint8_t> st0(stage_bytes), st1(stage_bytes);
    void* stage[2] = {st0.data(), st1.data()};
    std::atomic<uint64_t> queued[2] = {{0}, {0}}, finished[2] = {{0}, {0}};
    std::mutex m;
    std::condition_variable cv;
    {
        AsyncQueue stream;
        const int rc = wfa::host::staged_copy(
            dst.data(), src.data(), bytes, stage, stage_bytes,
            [&](void* d, const void* staged, size_t n, int b) {
                const uint64_t ticket = ++queued[b];
                stream.push([&, d, staged, n, b, ticket] {
                    memcpy(d, staged, n);  // reads the staging buffer LATER: a ring that refills it too early corrupts dst
                    { std::lock_guard<std::mutex> l(m); finished[b] = ticket; }
                    cv.notify_all();
                });
                return 0;
            },
            [&](int b) {
                std::unique_lock<std::mutex> l(m);
                cv.wait(l, [&] { return finished[b].load() == queued[b].load(); });
                return 0;
            },
            /*serial_below=*/stage_bytes / 2);  // small enough for the copy threads to take part
        if (rc) return 1;
    }  // the queue drains here (hipStreamSynchronize)
    if (bytes && memcmp(src.data(), dst.data(), bytes) != 0) { fprintf(stderr, "staged copy differs from its source\n"); return 1; }
    printf("{\"bytes\": %zu, \"stage_bytes\": %zu, \"chunks\": %zu}\n", bytes, stage_bytes, (bytes + stage_bytes - 1) / stage_bytes);
    return 0;
}

// File: cases back to back, each int64 R, int64 have_u16, then the columns off[R] (int64), len[R] (int32), pol[R] (int8).
// Every column is an exactly-sized heap copy: a read past the last record is a heap-buffer-overflow for the sanitizer.
int check_layout(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    printf("{\"layouts\": [");
    int64_t head[2];
    int n_cases = 0;
    while (fread(head, sizeof(int64_t), 2, f) == 2) {
        const size_t R = (size_t)head[0];
        int64_t* off = (int64_t*)malloc(R ? R * sizeof(int64_t) : 1);  // R == 0: one byte nobody may read
        int32_t* len = (int32_t*)malloc(R ? R * sizeof(int32_t) : 1);
        int8_t* pol = (int8_t*)malloc(R ? R : 1);
        if (!off || !len || !pol) return 2;
        if (fread(off, sizeof(int64_t), R, f) != R || fread(len, sizeof(int32_t), R, f) != R || fread(pol, 1, R, f) != R) {
            fprintf(stderr, "case %d is cut short\n", n_cases);
            return 2;
        }
        const bool uniform = wfa::host::records_uniform((int64_t)R, off, len, pol);
        const wfa::UniformLayout u = wfa::host::uniform_layout(uniform, (int64_t)R, R ? len[0] : 0, R ? off[0] : 0,
                                                               R ? pol[0] : (int8_t)0, head[1] != 0);
        printf("%s[%d, %d, %d, %d, %d, %d, %lld]", n_cases ? ", " : "", (int)uniform, (int)u.span, (int)u.pad, (int)u.positive,
               (int)u.L, (int)u.S, (long long)u.off0);
        free(off); free(len); free(pol);
        ++n_cases;
    }
    fclose(f);
    printf("], \"cases\": %d}\n", n_cases);
    return 0;
}

// File: int32 triples (start, end, max_len).  Prints the clamped window of each, and for each the largest sample index a
// wave-strided kernel loop (`for (i = start + lane; i < e; i += 64)`, lane 0..63, e = min(end, L) for an L <= max_len)
// computes, in 64 bits: the test asserts it fits an int32 with room to spare.
int check_window(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    printf("{\"windows\": [");
    int32_t t[3];
    int n_cases = 0;
    while (fread(t, sizeof(int32_t), 3, f) == 3) {
        const wfa::host::BaselineWindow w = wfa::host::baseline_window(t[0], t[1], t[2]);
        const int first = w.start + 63;                       // the addition the kernels do: int, under the sanitizer
        const int64_t last = (int64_t)(w.end > first ? w.end : first) + 64;
        printf("%s[%d, %d, %lld]", n_cases ? ", " : "", (int)w.start, (int)w.end, (long long)last);
        ++n_cases;
    }
    fclose(f);
    printf("], \"cases\": %d}\n", n_cases);
    return 0;
}

// k_dense_unpack on the host: every lane of every batch of one upload, the way wfa_upload_dense_rows cuts it.  Each
// batch is an exactly-sized, 16-byte aligned heap copy of its rows and the pool holds exactly n_rows * L elements: a
// load outside the batch buffer or a store outside the pool is a heap-buffer-overflow, a load the alignment does not
// allow a misaligned-address report.  Returns the elements that differ from rows[r].wave[j] (0 = pass); *negative = the
// smallest row the lanes reported (-1: none).
template <int ES, bool SIGNED>
int64_t dense_upload(const std::vector<uint8_t>& rows, int64_t n_rows, int64_t row_bytes, int64_t wave_offset, int64_t L,
                     int64_t batch_bytes, int64_t* negative, int64_t* lanes) {
    namespace H = wfa::host;
    const int W = H::dense_load_bytes(wave_offset, row_bytes, ES);
    const size_t pool_bytes = (size_t)(n_rows * L) * ES;
    uint8_t* pool = (uint8_t*)malloc(pool_bytes ? pool_bytes : 1);  // malloc: 16-byte aligned, exactly sized
    if (!pool) return -1;
    memset(pool, 0xa5, pool_bytes);
    *negative = -1;
    const int64_t rpb = n_rows && L ? H::dense_rows_per_batch(n_rows, row_bytes, batch_bytes) : 1;
    for (int64_t row = 0; row < n_rows && L > 0; row += rpb) {
        const int64_t nr = rpb < n_rows - row ? rpb : n_rows - row;
        const size_t bytes = (size_t)(nr * row_bytes);
        uint8_t* buf = (uint8_t*)malloc(bytes);
        memcpy(buf, rows.data() + (size_t)(row * row_bytes), bytes);
        H::DenseBatch b{};
        b.out_begin = (uint64_t)(row * L);
        b.out_end = (uint64_t)((row + nr) * L);
        b.row0 = row;
        b.L = (uint32_t)L;
        b.row_elems = (uint32_t)(row_bytes / ES);
        b.wave_elem = (uint32_t)(wave_offset / ES);
        const uint64_t c0 = H::dense_first_chunk(b, ES), nc = H::dense_chunk_count(b, ES);
        for (uint64_t g = 0; g < nc; ++g) {
            int64_t neg = -1;
            switch (W) {
                case 2: if constexpr (ES == 2) neg = H::dense_unpack_lane<ES, 2, SIGNED>(buf, pool, b, c0 + g); break;
                case 4: neg = H::dense_unpack_lane<ES, 4, SIGNED>(buf, pool, b, c0 + g); break;
                case 8: neg = H::dense_unpack_lane<ES, 8, SIGNED>(buf, pool, b, c0 + g); break;
                default: neg = H::dense_unpack_lane<ES, 16, SIGNED>(buf, pool, b, c0 + g); break;
            }
            if (neg >= 0 && (*negative < 0 || neg < *negative)) *negative = neg;
        }
        *lanes += (int64_t)nc;
        free(buf);
    }
    int64_t bad = 0;
    for (int64_t r = 0; r < n_rows; ++r)
        for (int64_t j = 0; j < L; ++j)
            bad += memcmp(pool + (size_t)(r * L + j) * ES, rows.data() + (size_t)(r * row_bytes + wave_offset + j * ES), ES) != 0;
    free(pool);
    return bad;
}

// Shapes (n, L) x layouts (wave at byte 76 / 0 / 2, and a 16-byte aligned one) x batch sizes (one row, three rows,
// everything) x element types, pseudo-random contents; for int16 one run per case with a few sign bits set.
int check_dense() {
    const int64_t shapes[][2] = {{0, 5}, {3, 0}, {1, 1}, {3, 7}, {5, 8}, {4, 9}, {7, 33}, {64, 800}, {9, 16}, {2, 4099}};
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&] { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    int64_t cases = 0, lanes = 0, widths[17] = {0};
    for (auto& sh : shapes) {
        const int64_t n = sh[0], L = sh[1];
        for (int es : {2, 4}) {
            const int64_t layouts[][2] = {{76, 76 + L * es}, {0, L * es}, {es == 2 ? 2 : 4, (es == 2 ? 2 : 4) + L * es},
                                          {32, (32 + L * es + 15) / 16 * 16}, {8, 8 + L * es + (L * es) % 8}};
            for (auto& lay : layouts) {
                const int64_t off = lay[0], rb = lay[1];
                if (rb == 0) continue;
                std::vector<uint8_t> rows((size_t)(n * rb));
                for (auto& x : rows) x = (uint8_t)next();
                if (es == 2)  // int16 contents without a sign bit
                    for (int64_t r = 0; r < n; ++r)
                        for (int64_t j = 0; j < L; ++j) rows[(size_t)(r * rb + off + 2 * j + 1)] &= 0x7f;
                for (int64_t batch : {(int64_t)1, 3 * rb, (int64_t)1 << 30}) {
                    int64_t neg = -1, bad;
                    ++widths[wfa::host::dense_load_bytes(off, rb, es)];
                    if (es == 4) bad = dense_upload<4, false>(rows, n, rb, off, L, batch, &neg, &lanes);
                    else bad = dense_upload<2, true>(rows, n, rb, off, L, batch, &neg, &lanes);
                    if (bad || neg != -1) { fprintf(stderr, "dense n=%lld L=%lld es=%d off=%lld rb=%lld batch=%lld: %lld bad, negative %lld\n", (long long)n, (long long)L, es, (long long)off, (long long)rb, (long long)batch, (long long)bad, (long long)neg); return 1; }
                    ++cases;
                    if (es == 2 && n > 0 && L > 0) {  // sign bits: last sample of the last row, then also a row in between
                        std::vector<uint8_t> marked = rows;
                        marked[(size_t)((n - 1) * rb + off + 2 * (L - 1) + 1)] |= 0x80;
                        bad = dense_upload<2, true>(marked, n, rb, off, L, batch, &neg, &lanes);
                        if (bad || neg != n - 1) { fprintf(stderr, "dense: negative in the last row reported as %lld\n", (long long)neg); return 1; }
                        const int64_t mid = n / 2;
                        marked[(size_t)(mid * rb + off + 1)] |= 0x80;
                        bad = dense_upload<2, true>(marked, n, rb, off, L, batch, &neg, &lanes);
                        if (bad || neg != mid) { fprintf(stderr, "dense: negative in row %lld reported as %lld\n", (long long)mid, (long long)neg); return 1; }
                        bad = dense_upload<2, false>(marked, n, rb, off, L, batch, &neg, &lanes);  // the same bits as uint16
                        if (bad || neg != -1) { fprintf(stderr, "dense: uint16 rows reported a negative\n"); return 1; }
                        cases += 3;
                    }
                }
            }
        }
    }
    printf("{\"cases\": %lld, \"lanes\": %lld, \"load2\": %lld, \"load4\": %lld, \"load8\": %lld, \"load16\": %lld}\n", (long long)cases,
           (long long)lanes, (long long)widths[2], (long long)widths[4], (long long)widths[8], (long long)widths[16]);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "dense")) return check_dense();
    if (argc == 3 && !strcmp(argv[1], "v1725")) return check_v1725(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "v1725-prefixes")) return check_v1725_prefixes(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "ring")) return check_ring((size_t)atoll(argv[2]), (size_t)atoll(argv[3]));
    if (argc == 3 && !strcmp(argv[1], "layout")) return check_layout(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "window")) return check_window(argv[2]);
    fprintf(stderr, "usage: host_check v1725 <blob> | v1725-prefixes <blob> | ring <bytes> <stage bytes> | layout <cases> | "
                    "window <cases>\n");
    return 2;
}
