// g++ build of deltaconv_amd/csrc/fps_math.h -- a serial emulation of fps_sample_global_kernel (fps.hip), the sampling kernel of
// the device geodesic farthest-point sampler for clouds above the LDS kernel's cap: D as 64-bit patterns in a plain array lowered
// by an unsigned minimum, the two frontier bit sets of exactly bitset_words(n) words scanned by word with zero words skipped, the
// read of D[v] in front of the minimum, the same (value, index) arg-max combine (tests/test_fps_large_host.py).  The graph stage is
// the one kernel both samplers share; its emulation is a copy of tests/hostcheck_fps' so that this directory builds alone.  Built
// twice: as a shared library for the test, and with -DHOSTCHECK_FPS_LARGE_MAIN as a stand-alone program (address +
// undefined-behaviour sanitizers) that checks the emulation against a heap Dijkstra of its own.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "../../deltaconv_amd/csrc/fps_math.h"

namespace {

typedef unsigned long long u64;
u64 bits_of(double v) { u64 b; memcpy(&b, &v, 8); return b; }
double value_of(u64 b) { double v; memcpy(&v, &b, 8); return v; }

}  // namespace

extern "C" {

int hfl_k() { return dcfps::K; }
int hfl_max_points() { return dcfps::LARGE_MAX_POINTS; }
int hfl_bitset_words(int32_t n) { return dcfps::bitset_words(n); }
uint64_t hfl_lds_bytes(int32_t n) { return dcfps::large_lds_bytes(n); }
uint64_t hfl_workspace_bytes(int64_t N) { return dcfps::large_workspace_bytes(N); }

// fps_knn_kernel: one query at a time, candidates by ascending index.  nbr [n,10] (-1 in unfilled slots), w [n,10] (+inf there)
void hfl_knn(const double* pos, int32_t n, int32_t* nbr, double* w) {
    for (int i = 0; i < n; ++i) {
        double d[dcfps::K];
        int id[dcfps::K];
        dcfps::topk_clear(d, id);
        for (int j = 0; j < n; ++j) {
            const double d2 = dcfps::dist2(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pos[3 * j], pos[3 * j + 1], pos[3 * j + 2]);
            if (j != i) dcfps::topk_insert(d, id, d2, j);
        }
        for (int s = 0; s < dcfps::K; ++s) {
            nbr[(size_t)i * dcfps::K + s] = id[s];
            w[(size_t)i * dcfps::K + s] = std::sqrt(d[s]);
        }
    }
}

// fps_sample_global_kernel: the rounds of one cloud.  sweeps (may be null): the number of sweeps of every round, [n_samples]
void hfl_sample(int32_t n, const int32_t* nbr, const double* w, int32_t start, int32_t n_samples, int32_t* out, int32_t* sweeps) {
    const int kk = n - 1 < dcfps::K ? n - 1 : dcfps::K;
    const int words = dcfps::bitset_words(n);
    std::vector<u64> D(n, bits_of(dcfps::inf()));
    std::vector<uint32_t> set_a(words, 0u), set_b(words, 0u);        // exactly `words` each: a step past a word edge is out of bounds
    uint32_t *cur = set_a.data(), *nxt = set_b.data();
    int src = start;
    out[0] = src;
    if (sweeps) sweeps[0] = 0;
    for (int r = 1; r < n_samples; ++r) {
        D[src] = 0ull;
        cur[src >> 5] = 1u << (src & 31);
        int count = 0;
        for (;;) {
            bool lowered = false;
            for (int wd = words - 1; wd >= 0; --wd) {                // any order of the words: the fixed point is the same
                uint32_t bits = cur[wd];
                if (!bits) continue;
                cur[wd] = 0u;
                do {
                    const int u = (wd << 5) + __builtin_ctz(bits);
                    bits &= bits - 1;
                    if (u >= n) { out[0] = -1; return; }             // a bit past the cloud: never set
                    const double du = value_of(D[u]);
                    for (int s = 0; s < kk; ++s) {
                        const int v = nbr[(size_t)u * dcfps::K + s];
                        if (v < 0 || v >= n) continue;
                        const u64 nd = bits_of(dcfps::relax(du, w[(size_t)u * dcfps::K + s]));
                        if (!(nd < D[v])) continue;                  // the read in front of the minimum
                        const u64 old = D[v];
                        D[v] = nd < old ? nd : old;                  // the minimum; it returns the value it met
                        if (nd < old) {
                            nxt[v >> 5] |= 1u << (v & 31);
                            lowered = true;
                        }
                    }
                } while (bits);
            }
            ++count;
            uint32_t* t = cur; cur = nxt; nxt = t;
            if (!lowered) break;
        }
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int u = n - 1; u >= 0; --u) dcfps::argmax_combine(bv, bi, value_of(D[u]), u);   // any order: the combine keeps the first index
        src = bi;
        out[r] = src;
        if (sweeps) sweeps[r] = count;
    }
}

// both stages on one cloud (pos [n,3] fp64).  Returns 0, or -1 on bad arguments.
int hfl_fps(const double* pos, int32_t n, int32_t n_samples, int32_t start, int32_t* out) {
    if (!pos || !out || n < 1 || n > dcfps::LARGE_MAX_POINTS || n_samples < 1 || start < 0 || start >= n) return -1;
    std::vector<int32_t> nbr((size_t)n * dcfps::K);
    std::vector<double> w((size_t)n * dcfps::K);
    hfl_knn(pos, n, nbr.data(), w.data());
    hfl_sample(n, nbr.data(), w.data(), start, n_samples, out, nullptr);
    return 0;
}

}  // extern "C"

#ifdef HOSTCHECK_FPS_LARGE_MAIN
namespace {

// the host library's algorithm (csrc_host/fps.cpp), restated on the emulation's graph: lazy-deletion heap Dijkstra per round
std::vector<int32_t> dijkstra_fps(int n, const std::vector<int32_t>& nbr, const std::vector<double>& w, int start, int m) {
    using VP = std::pair<double, int>;
    const int kk = n - 1 < dcfps::K ? n - 1 : dcfps::K;
    std::vector<double> D(n, dcfps::inf());
    std::vector<int32_t> out(m);
    out[0] = start;
    for (int r = 1; r < m; ++r) {
        std::priority_queue<VP, std::vector<VP>, std::greater<VP>> q;
        D[out[r - 1]] = 0.0;
        q.push({0.0, out[r - 1]});
        while (!q.empty()) {
            const VP c = q.top();
            q.pop();
            for (int s = 0; s < kk; ++s) {
                const int v = nbr[(size_t)c.second * dcfps::K + s];
                const double nd = c.first + w[(size_t)c.second * dcfps::K + s];
                if (nd < D[v]) { D[v] = nd; q.push({nd, v}); }
            }
        }
        int best = 0;
        for (int j = 1; j < n; ++j)
            if (D[j] > D[best]) best = j;
        out[r] = best;
    }
    return out;
}

int check(const char* name, const std::vector<double>& pos, int m, int start) {
    const int n = (int)(pos.size() / 3);
    std::vector<int32_t> nbr((size_t)n * dcfps::K), got(m), sweeps(m);
    std::vector<double> w((size_t)n * dcfps::K);
    hfl_knn(pos.data(), n, nbr.data(), w.data());
    hfl_sample(n, nbr.data(), w.data(), start, m, got.data(), sweeps.data());
    const std::vector<int32_t> want = dijkstra_fps(n, nbr, w, start, m);
    int most = 0;
    for (int r = 0; r < m; ++r) {
        if (sweeps[r] > most) most = sweeps[r];
        if (got[r] != want[r]) {
            printf("FAIL %s: round %d picks %d, Dijkstra picks %d\n", name, r, got[r], want[r]);
            return 1;
        }
    }
    printf("ok %s: n = %d, %d samples, at most %d sweeps per round\n", name, n, m, most);
    return 0;
}

}  // namespace

int main() {
    uint64_t state = 0x9E3779B97F4A7C15ull;
    auto uniform = [&state]() {                                  // splitmix64 -> [0, 1)
        uint64_t z = (state += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
    };
    int bad = 0;
    std::vector<double> cloud(3 * 3000);
    for (double& v : cloud) v = uniform();
    auto first = [&cloud](int n) { return std::vector<double>(cloud.begin(), cloud.begin() + 3 * n); };
    bad += check("random 3000", cloud, 60, 5);
    bad += check("random 700", first(700), 120, 699);
    // bit-set word edges: the last vertex is the start, so the last bit of the last word is the first one set
    bad += check("n = 31", first(31), 31, 30);
    bad += check("n = 32", first(32), 32, 31);
    bad += check("n = 33", first(33), 33, 32);
    bad += check("n = 64", first(64), 64, 63);
    bad += check("n = 65", first(65), 65, 64);
    std::vector<double> grid;                                    // integer grid: ties everywhere
    for (int x = 0; x < 9; ++x)
        for (int y = 0; y < 9; ++y)
            for (int z = 0; z < 3; ++z) { grid.push_back(x); grid.push_back(y); grid.push_back(z); }
    bad += check("grid", grid, 243, 0);
    std::vector<double> twice = first(60);                       // every point twice
    twice.insert(twice.end(), cloud.begin(), cloud.begin() + 3 * 60);
    bad += check("duplicates", twice, 130, 3);
    std::vector<double> two;                                     // two clusters far apart: rounds with max(D) = +inf
    for (int i = 0; i < 30; ++i)
        for (int a = 0; a < 3; ++a) two.push_back(uniform() + (i >= 15 && a == 0 ? 100.0 : 0.0));
    bad += check("two clusters", two, 30, 2);
    bad += check("one point", std::vector<double>{1.0, 2.0, 3.0}, 4, 0);
    bad += check("seven points", first(7), 40, 6);
    std::vector<int32_t> out(3);
    if (hfl_fps(cloud.data(), 0, 3, 0, out.data()) != -1 || hfl_fps(cloud.data(), 5, 3, 5, out.data()) != -1 ||
        hfl_fps(cloud.data(), dcfps::LARGE_MAX_POINTS + 1, 3, 0, out.data()) != -1) {
        printf("FAIL argument checks\n");
        ++bad;
    }
    if (dcfps::bitset_words(1) != 1 || dcfps::bitset_words(32) != 1 || dcfps::bitset_words(33) != 2 ||
        dcfps::large_lds_bytes(dcfps::LARGE_MAX_POINTS) != 65536 ||
        dcfps::large_workspace_bytes(1000) < dcfps::workspace_bytes(1000) + 8000) {
        printf("FAIL sizes\n");
        ++bad;
    }
    printf(bad ? "hostcheck_fps_large: FAILED\n" : "hostcheck_fps_large: all ok\n");
    return bad ? 1 : 0;
}
#endif
