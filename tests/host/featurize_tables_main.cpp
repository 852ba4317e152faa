// tests/host/featurize_tables_main.cpp -- the featurizer's host tables (csrc/kws_featurize_tables.h) checked without a device:
// what the chunk cutter and the lane matching must deliver for the kernels to be right (every bank weight exactly once, at its
// bin) and fast (bank-conflict free starts).  tests/test_featurize_tables_host.py builds and runs it; tests/host/Makefile builds
// it under AddressSanitizer / UBSan.  `--dump-bank mel|bark` writes the default geometry's float32 bank to stdout instead.
#include "kws_featurize_tables.h"

using namespace kws;

struct Case { const char *name; double buffer_t, window_t, hop_t; int n_fft, n_filt, n_mfcc, use_delta, bank_kind; };
// the rows of tests/geometry_cases.py (mel bank), then the default geometry with both banks
static const Case kCases[] = {
    {"tuned-2", 0.1, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_MEL},  {"tuned-14", 0.5, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_MEL},
    {"tuned-61", 2.0, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_MEL}, {"tuned-45", 1.5, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_MEL},
    {"gen1-9", 0.2, 0.064, 0.016, 1024, 20, 20, 0, KWS_BANK_MEL},   {"gen1-48", 0.5, 0.025, 0.010, 1024, 40, 13, 0, KWS_BANK_MEL},
    {"gen1-48d", 0.5, 0.025, 0.010, 1024, 40, 13, 1, KWS_BANK_MEL}, {"rad2-48", 0.5, 0.025, 0.010, 512, 26, 13, 0, KWS_BANK_MEL},
    {"rad2-31", 1.0, 0.016, 0.032, 256, 13, 13, 0, KWS_BANK_MEL},   {"default-mel", 1.0, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_MEL},
    {"default-bark", 1.0, 0.064, 0.032, 1024, 20, 20, 0, KWS_BANK_BARK},
};

static const char *g_case = "";
static const char *g_table = "";
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s %s: %s: ", g_case, g_table, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fprintf(stderr, "\n");                                    \
            return false;                                                  \
        }                                                                  \
    } while (0)

static bool build(const Case &c, FeatTables &t)
{
    const kws_params p{c.buffer_t, c.window_t, c.hop_t, 16000, 2, c.n_fft, c.n_filt, c.n_mfcc, c.use_delta};
    kws_geometry g;
    std::string err;
    int rc = derive(&p, &g, err);
    if (!rc) rc = build_feat_tables(p, g, c.bank_kind, t, err);
    CHECK(rc == KWS_OK, "status %d: %s", rc, err.c_str());
    return true;
}

static bool check_chunks(const FeatTables &t, const ChunkTables &T, int n_bins, int n_filt, int align, bool mirrored)
{
    const int npos = mirrored ? kV3OffM + 256 : n_bins, chp = T.chp, nlog = T.nlog;
    std::vector<int> bin_of(npos, -1);
    for (int k = 0; k < n_bins; ++k) bin_of[mirrored ? v3_pos_of_bin(k) : k] = k;
    CHECK(nlog <= 64 && chp > 0 && chp % 4 == 0, "nlog %d chp %d", nlog, chp);
    CHECK((int)T.chunks.size() == 64 && T.w.size() == (size_t)64 * chp && (int)T.bcs.size() == n_filt + 1, "table sizes");
    CHECK(T.bcs[0] == 0 && T.bcs[n_filt] == nlog, "bcs ends %d, %d (nlog %d)", T.bcs[0], T.bcs[n_filt], nlog);
    for (int i = 0; i < n_filt; ++i) CHECK(T.bcs[i] <= T.bcs[i + 1], "bcs decreases at band %d", i);

    std::vector<int> hits((size_t)n_filt * n_bins, 0), owner_of(nlog, -1), idle_used(64, 0), residue[2] = {std::vector<int>(32, 0), std::vector<int>(32, 0)};
    int idle_left = 64 - nlog;
    for (int lane = 0; lane < 64; ++lane) {
        const TabInt4 ch = T.chunks[lane];
        CHECK(ch.y >= 0 && ch.y % align == 0, "lane %d starts at %d (align %d)", lane, ch.y, align);
        CHECK(ch.z >= 0 && ch.z < 64 && ch.w == 0, "lane %d chunk id %d", lane, ch.z);
        if (ch.z >= nlog) {      // an idle lane: an unused chunk id of its own, or 63 once they are all taken; no weights
            CHECK(!idle_used[ch.z] || (ch.z == 63 && idle_left == 0), "idle lane %d repeats chunk id %d", lane, ch.z);
            if (!idle_used[ch.z]) { idle_used[ch.z] = 1; --idle_left; }
            for (int k = 0; k < chp; ++k) CHECK(T.w[(size_t)lane * chp + k] == 0.f, "idle lane %d has a weight at %d", lane, k);
            continue;
        }
        CHECK(owner_of[ch.z] < 0, "chunk %d on lanes %d and %d", ch.z, owner_of[ch.z], lane);
        owner_of[ch.z] = lane;
        CHECK(ch.x >= 0 && ch.x < n_filt && ch.z >= T.bcs[ch.x] && ch.z < T.bcs[ch.x + 1], "chunk %d is not one of band %d", ch.z, ch.x);
        if (T.perfect) CHECK(residue[lane >> 5][(ch.y / align) & 31]++ == 0, "lane %d shares its LDS bank in its half-wave", lane);
        for (int k = 0; k < chp; ++k) {
            const float w = T.w[(size_t)lane * chp + k];
            if (w == 0.f) continue;
            const int pos = ch.y + k, bin = pos < npos ? bin_of[pos] : -1;
            CHECK(bin >= 0, "lane %d weight %d sits on position %d, which holds no bin", lane, k, pos);
            const double b = t.bank[(size_t)ch.x * n_bins + bin];
            const float want = mirrored ? (float)((double)(float)b / 4096.0) : (float)b;
            CHECK(b != 0.0 && w == want, "band %d bin %d: weight %.9g, bank gives %.9g", ch.x, bin, (double)w, (double)want);
            ++hits[(size_t)ch.x * n_bins + bin];
        }
    }
    for (int c = 0; c < nlog; ++c) CHECK(owner_of[c] >= 0, "chunk %d of %d has no lane", c, nlog);
    for (int i = 0; i < n_filt; ++i)
        for (int j = 0; j < n_bins; ++j)
            CHECK(hits[(size_t)i * n_bins + j] == (t.bank[(size_t)i * n_bins + j] != 0.0 ? 1 : 0), "band %d bin %d is gathered %d times", i, j,
                  hits[(size_t)i * n_bins + j]);
    return true;
}

static bool unit(const std::vector<TabCplx> &tw, const char *what)
{
    for (size_t k = 0; k < tw.size(); ++k)
        CHECK(std::fabs(std::hypot((double)tw[k].x, (double)tw[k].y) - 1.0) <= 1e-6, "%s[%zu] = (%g, %g)", what, k, (double)tw[k].x, (double)tw[k].y);
    return true;
}

static bool check_case(const Case &c)
{
    g_case = c.name;
    g_table = "";
    FeatTables t;
    if (!build(c, t)) return false;
    const int n_bins = c.n_fft / 2 + 1;
    g_table = "align 1";
    if (!check_chunks(t, t.T1, n_bins, c.n_filt, 1, false)) return false;
    g_table = c.n_fft == 1024 ? "align 2 mirrored" : "align 2";
    if (!check_chunks(t, t.T3, n_bins, c.n_filt, 2, c.n_fft == 1024)) return false;
    g_table = "";
    if (std::string(c.name) == "default-mel")   // v3_applies (kws_featurize.hip) needs this for the kernel the suite and the benchmark run
        CHECK(t.T1.perfect && t.T3.perfect && (t.T3.chp == 12 || t.T3.chp == 16 || t.T3.chp == 20), "perfect %d %d, mirrored chp %d", (int)t.T1.perfect,
              (int)t.T3.perfect, t.T3.chp);
    CHECK(t.dct.size() == (size_t)t.n_filt_pad * c.n_mfcc, "dct size");
    for (int n = 0; n < c.n_filt; ++n)
        CHECK(t.dct[(size_t)n * c.n_mfcc] == (float)std::sqrt(1.0 / c.n_filt), "dct[%d][0] = %.9g", n, (double)t.dct[(size_t)n * c.n_mfcc]);
    CHECK(t.tws.size() == 257 && t.tws3.size() == 256 && (int)t.twg.size() == c.n_fft / 2, "twiddle table sizes");
    return unit(t.tws, "tws") && unit(t.tws3, "tws3") && unit(t.twg, "twg");
}

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--dump-bank") {
        const bool bark = std::string(argv[2]) == "bark";
        FeatTables t;
        if (!build(kCases[bark ? 10 : 9], t)) return 1;
        return std::fwrite(t.bw.data(), sizeof(float), t.bw.size(), stdout) == t.bw.size() ? 0 : 1;
    }
    for (const Case &c : kCases)
        if (!check_case(c)) return 1;
    std::printf("featurize tables: %zu cases ok\n", sizeof(kCases) / sizeof(kCases[0]));
    return 0;
}
