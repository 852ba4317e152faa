// csrc/kws_featurize_tables.h -- everything the featurizer computes on the host: the frame geometry, the mel / bark bank, the chunk
// tables of the sparse band gather with their LDS-bank placement, the twiddles and the DCT (double precision, then rounded once), and
// the arena that lays the tables out for one device allocation.  No HIP here: the standard library and kws.h only, so that
// tests/host/featurize_tables_main.cpp holds all of it with a plain C++ compiler (and under a sanitizer) without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "kws.h"

#ifdef __HIPCC__
#define KWS_TABLES_HD __host__ __device__
#else
#define KWS_TABLES_HD
#endif

namespace kws {

constexpr int kMaxChunks = 64;
constexpr int kV3OffM = 320;                 // the mirrored half of the power spectrum: position kV3OffM + p holds bin 512 - p, p = 0..255
// pass-1 lane l of the tuned kernel (kws_featurize_v3.h) owns the input points sigma(l) + 64 a
KWS_TABLES_HD inline int v3_sigma(int l) { return 8 * (l & 7) + (l >> 3); }
// position of bin k in the wave's power planes
KWS_TABLES_HD inline int v3_pos_of_bin(int k) { return k <= 256 ? k : kV3OffM + 512 - k; }

// the layouts of HIP's float2 and int4, which is what the kernels read these tables as
struct TabCplx { float x, y; };
struct TabInt4 { int x, y, z, w; };

// the builders report an error as a kws_status and its text; the caller hands the text to fail() (kws_common.h)
inline int tab_fail(std::string &err, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

inline int derive(const kws_params *p, kws_geometry *g, std::string &err)
{
    if (!p || !g) return tab_fail(err, KWS_ERR_INVALID, "null params");
    if (p->sample_rate <= 0 || p->window_t <= 0 || p->hop_t <= 0 || p->buffer_t <= 0)
        return tab_fail(err, KWS_ERR_INVALID, "sample_rate/window_t/hop_t/buffer_t must be positive");
    // classifier/params.py:59-91
    g->window_samples = (int)(p->sample_rate * p->window_t + 0.5);
    g->hop_samples = (int)(p->sample_rate * p->hop_t + 0.5);
    g->max_samples = (int)(p->buffer_t * p->sample_rate);
    if (g->hop_samples <= 0 || g->window_samples <= 0) return tab_fail(err, KWS_ERR_INVALID, "window/hop round to zero samples");
    int samples = (int)(p->sample_rate * p->buffer_t + 0.5);
    g->buffer_samples = g->hop_samples * (samples / g->hop_samples);
    g->n_features = 1 + (int)std::floor((double)(g->buffer_samples - g->window_samples) / (double)g->hop_samples);
    g->feature_size = p->use_delta ? 2 * p->n_mfcc : p->n_mfcc;
    return KWS_OK;
}

// frames of a clip of max_samples; kws_featurizer_create refuses params where this differs from n_features
inline int clip_frames(const kws_geometry &g) { return (g.max_samples - g.window_samples) / g.hop_samples + 1; }

inline int build_mel_bank(int sample_rate, int n_fft, int n_filt, std::vector<double> &bank, std::string &err)
{
    // sonopy.filterbanks as restated by inference/tflite/mfcc.h:230-264; span 0..sample_rate
    // (inference/tflite/speech_commands.h:304-307)
    const int n_bins = n_fft / 2 + 1, n = n_filt + 2;
    std::vector<int> pts(n);
    const double lo = 1127.0 * std::log(1.0 + 0.0 / 700.0), hi = 1127.0 * std::log(1.0 + sample_rate / 700.0);
    const double step = (hi - lo) / (double)(n - 1);
    for (int i = 0; i < n; ++i) {
        const double m = (i == n - 1) ? hi : lo + i * step;
        pts[i] = (int)(700.0 * (std::exp(m / 1127.0) - 1.0) * n_bins / sample_rate);
    }
    for (int i = 1; i < n; ++i)
        if (pts[i] <= pts[i - 1])
            return tab_fail(err, KWS_ERR_UNSUPPORTED, "mel grid has repeated FFT bins for n_fft=%d n_filt=%d (sonopy's "
                                                      "duplicate-point correction is not implemented)", n_fft, n_filt);
    if (pts[n - 1] > n_bins) return tab_fail(err, KWS_ERR_INVALID, "mel grid exceeds the spectrum");
    bank.assign((size_t)n_filt * n_bins, 0.0);
    for (int i = 0; i < n_filt; ++i) {
        const int l = pts[i], m = pts[i + 1], r = pts[i + 2];
        for (int j = l; j < m; ++j) bank[(size_t)i * n_bins + j] = (double)(j - l) / (double)(m - l);
        for (int j = m; j < r; ++j) bank[(size_t)i * n_bins + j] = (double)(r - j) / (double)(r - m);
    }
    return KWS_OK;
}

inline int build_bark_bank(int sample_rate, int n_fft, int n_filt, std::vector<double> &bank, std::string &err)
{
    // common/bark_feature.py:92-136 with scale="constant".  The bin<->Hz maps at :112/:134 are
    // called with their DEFAULT nfft=512 and sample_rate=16000 whatever the caller passes; kept.
    const int n_bins = n_fft / 2 + 1, n = n_filt + 4;
    auto hz2bark = [](double f) { return 6.0 * std::asinh(f / 600.0); };
    auto bark2hz = [](double v) { return 600.0 * std::sinh(v / 6.0); };
    auto Fm = [](double fb, double fc) {
        if (fc - 2.5 <= fb && fb <= fc - 0.5) return std::pow(10.0, 2.5 * (fb - fc + 0.5));
        if (fc - 0.5 < fb && fb < fc + 0.5) return 1.0;
        if (fc + 0.5 <= fb && fb <= fc + 1.3) return std::pow(10.0, -2.5 * (fb - fc - 0.5));
        return 0.0;
    };
    const double lo = hz2bark(0.0), hi = hz2bark(sample_rate / 2.0), step = (hi - lo) / (double)(n - 1);
    std::vector<double> pt(n);
    std::vector<int> bins(n);
    for (int i = 0; i < n; ++i) {
        pt[i] = (i == n - 1) ? hi : lo + i * step;
        bins[i] = (int)std::floor(513.0 * bark2hz(pt[i]) / 16000.0);
    }
    bank.assign((size_t)n_filt * n_bins, 0.0);
    for (int i = 0; i < n_filt; ++i)
        for (int j = bins[i]; j < bins[i + 4]; ++j) {
            if (j < 0 || j >= n_bins) return tab_fail(err, KWS_ERR_INVALID, "bark bank needs bin %d but n_fft=%d has %d", j, n_fft, n_bins);
            bank[(size_t)i * n_bins + j] = std::fabs(Fm(hz2bark(j * 16000.0 / 513.0), pt[i + 2]));
        }
    return KWS_OK;
}

// Chunk tables for the sparse band gather: every band's span cut into <= 64 lane chunks.  `perfect`: the lane placement below found
// a bank-conflict free start for every chunk; otherwise the chunks keep their natural order (correct, just slower).
struct ChunkTables {
    int ch, chp, nlog;
    bool perfect;
    std::vector<TabInt4> chunks;   // [64 lanes] {band, first position read, chunk id, 0}
    std::vector<float> w;          // [64 lanes][chp]
    std::vector<int> bcs;          // [n_filt + 1] first chunk of each band
};

struct ChunkRun { int band, lo, hi; };       // positions [lo, hi) of one band
struct LogicalChunk { int band, a, len; };   // (band, first position, positions)

// Lane placement.  Every lane reads p[start + t] for the same t, so the 32 lanes of a half-wave hit different LDS banks
// iff their starts (in units of `align` bins) differ mod 32.  A chunk of `len` bins may start anywhere (on a multiple
// of `align`) in [a + len - chp, a] (the extra bins get zero weights), so: bipartite matching of chunks to the 64
// (half, residue) slots, lane = 32 * half + residue.  (Chunk starts taken as they come collide ~3-way on average:
// 29 % of the first kernel's LDS cycles were conflicts.)  Fills owner[lane] (chunk or -1) and start_of[chunk].
inline bool place_chunks(const std::vector<LogicalChunk> &logical, int chp, int align, std::vector<int> &start_of, std::vector<int> &owner)
{
    const int nlog = (int)logical.size();
    start_of.assign(nlog, 0);
    owner.assign(64, -1);
    std::vector<std::vector<std::pair<int, int>>> cand(nlog);          // (slot, start)
    for (int c = 0; c < nlog; ++c)
        for (int st = logical[c].a - logical[c].a % align; st >= std::max(0, logical[c].a + logical[c].len - chp); st -= align)
            for (int h = 0; h < 2; ++h) cand[c].push_back({32 * h + ((st / align) & 31), st});
    std::vector<int> owner_start(64, 0);
    std::function<bool(int, std::vector<char> &)> place = [&](int c, std::vector<char> &seen) -> bool {
        for (auto &e : cand[c]) {
            if (seen[e.first]) continue;
            seen[e.first] = 1;
            if (owner[e.first] < 0 || place(owner[e.first], seen)) {
                owner[e.first] = c; owner_start[e.first] = e.second;
                return true;
            }
        }
        return false;
    };
    bool perfect = nlog <= 64;
    for (int c = 0; c < nlog && perfect; ++c) {
        std::vector<char> seen(64, 0);
        perfect = place(c, seen);
    }
    if (perfect) {
        for (int sl = 0; sl < 64; ++sl)
            if (owner[sl] >= 0) start_of[owner[sl]] = owner_start[sl];
    } else {                                                           // keep the natural order (correct, just slower)
        std::fill(owner.begin(), owner.end(), -1);
        for (int c = 0; c < nlog && c < 64; ++c) { start_of[c] = logical[c].a - logical[c].a % align; owner[c] = c; }
    }
    return perfect;
}

// `align` = 1: a lane reads its bins one per LDS instruction (first-generation kernel); 2: chunks start on even positions so that two
// bins come per ds_read_b64 (kws_featurize_v3.h).
// `mirrored` (third-generation kernel): the chunks run over POSITIONS of the wave's two power planes (v3_pos_of_bin: bins 0..256 in
// place, bins 257..512 in descending order behind them), a band's span splits into at most two runs of consecutive positions, and the
// weights carry the factor 2^-12 the kernel leaves out of its power spectrum
inline ChunkTables build_chunks(const std::vector<double> &bank, int n_bins, int n_filt, const std::vector<int> &first,
                                const std::vector<int> &width, int align, bool mirrored)
{
    ChunkTables T;
    const int npos = mirrored ? kV3OffM + 256 : n_bins;
    std::vector<int> bin_of(npos, -1);
    for (int k = 0; k < n_bins; ++k) bin_of[mirrored ? v3_pos_of_bin(k) : k] = k;
    const double wscale = mirrored ? 1.0 / 4096.0 : 1.0;
    std::vector<ChunkRun> runs;
    for (int i = 0; i < n_filt; ++i) {
        if (width[i] <= 0) continue;
        if (!mirrored) { runs.push_back(ChunkRun{i, first[i], first[i] + width[i]}); continue; }
        const int a = first[i], z = first[i] + width[i] - 1;
        if (a <= 256) runs.push_back(ChunkRun{i, a, std::min(z, 256) + 1});
        if (z >= 257) runs.push_back(ChunkRun{i, v3_pos_of_bin(z), v3_pos_of_bin(std::max(a, 257)) + 1});
    }
    int ch = align;
    for (;; ch += align) {
        int cnt = 0;
        for (const ChunkRun &r : runs) cnt += ((r.hi - r.lo) + (r.lo % align) + ch - 1) / ch;
        if (cnt <= kMaxChunks) break;
    }
    const int chp = (ch + 3) & ~3;
    // logical chunks in band order; chunk boundaries sit on multiples of `align`
    std::vector<LogicalChunk> logical;
    std::vector<int> bcs(n_filt + 1, 0);
    size_t ri = 0;
    for (int i = 0; i < n_filt; ++i) {
        bcs[i] = (int)logical.size();
        for (; ri < runs.size() && runs[ri].band == i; ++ri) {
            const int s0 = runs[ri].lo - runs[ri].lo % align, end = runs[ri].hi;
            for (int lo = s0; lo < end; lo += ch) {
                const int a = std::max(lo, runs[ri].lo), z = std::min(lo + ch, end);
                if (z > a) logical.push_back(LogicalChunk{i, a, z - a});
            }
        }
    }
    bcs[n_filt] = (int)logical.size();
    const int nlog = (int)logical.size();
    std::vector<int> start_of, owner;
    T.perfect = place_chunks(logical, chp, align, start_of, owner);
    // per-lane tables (always 64 lanes): {band, start, chunk id, 0} and chp weights; idle lanes take the unused chunk ids
    T.chunks.assign(64, TabInt4{0, 0, 0, 0});
    T.w.assign((size_t)64 * chp, 0.f);
    int spare = nlog;
    for (int lane = 0; lane < 64; ++lane) {
        const int c = owner[lane];
        if (c < 0) { T.chunks[lane] = TabInt4{0, 0, spare < 64 ? spare++ : 63, 0}; continue; }
        T.chunks[lane] = TabInt4{logical[c].band, start_of[c], c, 0};
        for (int t = 0; t < chp; ++t) {
            const int pos = start_of[c] + t;
            if (pos >= logical[c].a && pos < logical[c].a + logical[c].len && pos < npos && bin_of[pos] >= 0)
                T.w[(size_t)lane * chp + t] = (float)((double)(float)bank[(size_t)logical[c].band * n_bins + bin_of[pos]] * wscale);
        }
    }
    T.ch = ch; T.chp = chp; T.nlog = nlog; T.bcs = bcs;
    return T;
}

// W_den^num = exp(-2 pi i num / den)
inline TabCplx twiddle(double num, double den)
{
    const double a = -2.0 * M_PI * num / den;
    return TabCplx{(float)std::cos(a), (float)std::sin(a)};
}

// every table of one featurizer (the comments of FeatDev, kws_featurize.hip, say how the kernels read them)
struct FeatTables {
    int n_frames, window_eff, n_filt_pad, log2n, tail_batch;
    std::vector<double> bank;                         // [n_filt][n_bins]
    std::vector<int> first, width;                    // [n_filt] band spans
    ChunkTables T1, T3;                               // align 1; align 2, mirrored when n_fft == 1024
    std::vector<TabCplx> tw1, tw2, tws, tw1s, tws3;   // n_fft = 1024 kernels
    std::vector<TabCplx> twg;                         // [n_fft/2] generic path
    std::vector<float> bw, dct;                       // the bank in float; [n_filt_pad][n_out] ortho DCT-II, zero rows past n_filt
};

// p has passed kws_featurizer_create's checks (n_filt 1..64, n_mfcc 1..n_filt, n_fft a power of two) and g = derive(p)
inline int build_feat_tables(const kws_params &p, const kws_geometry &g, int bank_kind, FeatTables &t, std::string &err)
{
    const int n_fft = p.n_fft, n_bins = n_fft / 2 + 1, n_filt = p.n_filt, n_out = p.n_mfcc;
    const int rc = bank_kind == KWS_BANK_MEL ? build_mel_bank(p.sample_rate, n_fft, n_filt, t.bank, err)
                                             : build_bark_bank(p.sample_rate, n_fft, n_filt, t.bank, err);
    if (rc) return rc;
    // sparse tables: per band the span [first non-zero, last non-zero] (width 0: an empty band), cut into <= 64 lane chunks
    t.first.assign(n_filt, 0);
    t.width.assign(n_filt, 0);
    for (int i = 0; i < n_filt; ++i) {
        int a = -1, z = -1;
        for (int j = 0; j < n_bins; ++j)
            if (t.bank[(size_t)i * n_bins + j] != 0.0) { if (a < 0) a = j; z = j; }
        if (a >= 0) { t.first[i] = a; t.width[i] = z - a + 1; }
    }
    t.T1 = build_chunks(t.bank, n_bins, n_filt, t.first, t.width, 1, false);
    t.T3 = build_chunks(t.bank, n_bins, n_filt, t.first, t.width, 2, n_fft == 1024);   // the position map is the 513-bin one

    t.tw1.resize(7 * 64); t.tw2.resize(7 * 8); t.tws.resize(257); t.tw1s.resize(7 * 64); t.tws3.resize(4 * 64);
    for (int k = 1; k < 8; ++k)
        for (int l = 0; l < 64; ++l) {
            t.tw1[(k - 1) * 64 + l] = twiddle((double)(l * k), 512.0);
            t.tw1s[(k - 1) * 64 + l] = twiddle((double)(v3_sigma(l) * k), 512.0);
        }
    for (int k = 1; k < 8; ++k)
        for (int l = 0; l < 8; ++l) t.tw2[(k - 1) * 8 + l] = twiddle((double)(l * k), 64.0);
    for (int k = 0; k <= 256; ++k) t.tws[k] = twiddle((double)k, 1024.0);
    for (int i = 0; i < 4 * 64; ++i) t.tws3[i] = twiddle((double)i, 1024.0);
    t.twg.resize((size_t)n_fft / 2);
    for (int k = 0; k < n_fft / 2; ++k) t.twg[k] = twiddle((double)k, (double)n_fft);

    t.bw.resize(t.bank.size());
    for (size_t i = 0; i < t.bank.size(); ++i) t.bw[i] = (float)t.bank[i];
    t.n_filt_pad = (n_filt + 3) & ~3;
    t.dct.assign((size_t)t.n_filt_pad * n_out, 0.f);
    for (int n = 0; n < n_filt; ++n)
        for (int k = 0; k < n_out; ++k)  // scipy dct type II norm='ortho' (bark_feature.py:172, mfcc.h:55-67)
            t.dct[(size_t)n * n_out + k] = (float)(std::cos(M_PI * (n + 0.5) * k / n_filt) * (k == 0 ? std::sqrt(1.0 / n_filt) : std::sqrt(2.0 / n_filt)));

    t.n_frames = clip_frames(g);
    t.window_eff = std::min(g.window_samples, n_fft);  // np.fft.rfft(frames, n): crop or zero-pad (bark_feature.py:87)
    t.log2n = 0;
    while ((1 << t.log2n) < n_fft) ++t.log2n;
    t.tail_batch = std::max(1, std::min(4, 64 / std::max(t.n_filt_pad, n_out)));
    return KWS_OK;
}

// The tables of one device allocation: add() appends a table to the host image at a 256-byte aligned offset (an empty table still
// takes `min_count` elements) and remembers which device pointer reads it; bind() sets those pointers once the image sits at `base`.
struct TableArena {
    struct Slot { void *field; size_t off; void (*set)(void *, unsigned char *); };
    std::vector<unsigned char> image;
    std::vector<Slot> slots;

    template <typename T, typename D> void add(const std::vector<T> &v, const D **field, size_t min_count = 0)
    {
        static_assert(sizeof(T) == sizeof(D), "the device reads the table's elements as they are");
        const size_t off = image.size();
        image.resize((off + std::max(v.size(), min_count) * sizeof(T) + 255) & ~(size_t)255, 0);
        if (!v.empty()) std::memcpy(image.data() + off, v.data(), v.size() * sizeof(T));
        slots.push_back(Slot{field, off, [](void *f, unsigned char *p) { *static_cast<const D **>(f) = reinterpret_cast<const D *>(p); }});
    }
    void bind(void *base) const
    {
        for (const Slot &s : slots) s.set(s.field, static_cast<unsigned char *>(base) + s.off);
    }
};

}  // namespace kws
