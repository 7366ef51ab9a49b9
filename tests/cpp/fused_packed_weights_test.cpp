// The vertex weights of the fused step as 16-bit offsets (qgd_setup.cpp packFusedWeights, FusedBlocks::vW16 / wRef; CPU only, compiled by
// tests/test_fused_packed_weights_host.py with plain g++ from the library's own host sources).
//   * uniform boxes and a slab shard QUALIFY: capPE == 8 and every weight's bit pattern within 65 535 of every other's.  Every entry of vW16,
//     decoded (reference + offset, taken as a double), is the vertex kernel's weight s.pcW bit for bit; entries beyond a vertex's count are
//     0; a box whose spacings are no powers of two has offsets other than 0; the reference is the same built with 1 and with 4 threads; the
//     default call keeps the full table next to the packed one, keepFullWeights = false drops it.
//   * the RULE on weight sets written by hand: a spread of exactly 65 535 packs and 65 536 does not; a set that straddles 0.125 -- where the
//     exponent changes and the spacing of the doubles halves -- decodes exactly; capPE != 8 does not pack; a vertex of count 0 is not looked at.
//   * a jittered mesh and a 2:1 graded box do NOT pack: no vW16, packedW == 0, and the full table is kept whatever the caller asked for.
//   * QGD_FUSED_PACKED_W=0 keeps the full table alone on a mesh that would pack.
#include <omp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "qgd_mesh.hpp"
#include "qgd_setup.hpp"

using namespace qgd;

static int fails = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (fails < 20) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++fails;                                       \
        }                                                  \
    } while (0)

static int64_t bitsOf(double w) { int64_t b; std::memcpy(&b, &w, 8); return b; }
static double fromBits(int64_t b) { double w; std::memcpy(&w, &b, 8); return w; }

// every entry of the packed table against the vertex kernel's own weights; returns the largest |offset|
static int checkPacked(const char* tag, const StaticData& s, const FusedBlocks& B) {
    int maxOff = 0;
    int64_t weights = 0;
    CHECK(B.vW16.size() == (size_t)B.nBlocks * B.capV * 8, "%s: %zu offsets for %d blocks of %d vertices", tag, B.vW16.size(), B.nBlocks, B.capV);
    if (B.vW16.size() != (size_t)B.nBlocks * B.capV * 8) return 0;
    for (int32_t b = 0; b < B.nBlocks; ++b) {
        const int32_t nV = B.hdr[4 * b + 2];
        for (int32_t lv = 0; lv < B.capV; ++lv) {
            const int n = lv < nV ? B.vCount[(size_t)b * B.capV + lv] : 0;
            const int16_t* off = &B.vW16[((size_t)b * B.capV + lv) * 8];
            for (int e = n; e < 8; ++e) CHECK(off[e] == 0, "%s: block %d vertex %d padded entry %d is %d", tag, b, lv, e, (int)off[e]);
            if (n == 0) continue;
            const int32_t v = B.verts[(size_t)b * B.capV + lv];
            const size_t base = (size_t)s.pcSlice[v >> 6] * 64 + (v & 63);
            for (int e = 0; e < n; ++e) {
                const double w = fusedWeightFromOffset(B.wRef, off[e]);
                CHECK(bitsOf(w) == bitsOf(s.pcW[base + (size_t)e * 64]), "%s: block %d vertex %d weight %d: %.17g decoded, %.17g in the mesh's table", tag, b, v, e, w,
                      s.pcW[base + (size_t)e * 64]);
                maxOff = std::max(maxOff, std::abs((int)off[e]));
                ++weights;
            }
        }
    }
    std::printf("%s: %lld weights as offsets from %.17g, largest |offset| %d\n", tag, (long long)weights, fromBits(B.wRef), maxOff);
    return maxOff;
}

static void qualifies(const char* tag, HostMesh& m, bool wantNonZero) {
    if (m.magSf.empty()) m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    omp_set_num_threads(4);
    const FusedBlocks B = buildFusedBlocks(s);
    CHECK(B.nBlocks > 0 && B.capPE == 8, "%s: %d blocks, capPE %d", tag, B.nBlocks, B.capPE);
    CHECK(B.packedW == 1, "%s does not pack", tag);
    if (B.packedW != 1) return;
    CHECK(B.vW.size() == (size_t)B.nBlocks * B.capPE * B.capV, "%s: the default call keeps the full table", tag);
    const int maxOff = checkPacked(tag, s, B);
    CHECK(!wantNonZero || maxOff > 0, "%s: every offset is 0", tag);
    omp_set_num_threads(1);
    const FusedBlocks B1 = buildFusedBlocks(s, false);
    omp_set_num_threads(4);
    CHECK(B1.packedW == 1 && B1.wRef == B.wRef, "%s: reference %lld with one thread, %lld with four", tag, (long long)B1.wRef, (long long)B.wRef);
    CHECK(B1.vW16 == B.vW16, "%s: the offsets differ between one thread and four", tag);
    CHECK(B1.vW.empty(), "%s: keepFullWeights = false keeps %zu doubles", tag, B1.vW.size());
}

static void doesNotQualify(const char* tag, HostMesh& m) {
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    for (int keep = 0; keep < 2; ++keep) {
        const FusedBlocks B = buildFusedBlocks(s, keep != 0);
        CHECK(B.nBlocks > 0, "%s: no blocks", tag);
        CHECK(B.packedW == 0 && B.vW16.empty() && B.wRef == 0, "%s packs", tag);
        CHECK(B.vW.size() == (size_t)B.nBlocks * B.capPE * B.capV && !B.vW.empty(), "%s: the full table is not kept (keepFullWeights %d)", tag, keep);
    }
    std::printf("%s: not packed, full table kept\n", tag);
}

// one block of capV vertices with eight weights each, patterns lo .. lo + spread spread over the entries (both ends present)
static FusedBlocks handMade(int capPE, int64_t lo, int64_t spread) {
    FusedBlocks B;
    B.nBlocks = 1; B.capV = 16; B.capPE = capPE;
    B.vCount.assign((size_t)B.capV, (uint8_t)std::min(capPE, 8));
    B.vW.assign((size_t)capPE * B.capV, 0.0);
    const int n = std::min(capPE, 8) * B.capV;
    for (int i = 0; i < n; ++i) {
        const int e = i / B.capV, lv = i % B.capV;
        const int64_t b = i == 0 ? lo : (i == n - 1 ? lo + spread : lo + (spread * i) / n);
        B.vW[(size_t)e * B.capV + lv] = fromBits(b);
    }
    return B;
}
static void checkHandMade(const char* tag, FusedBlocks& B, bool want) {
    const RawVec<double> vW = B.vW;
    const bool got = packFusedWeights(B);
    CHECK(got == want && (B.packedW == 1) == want, "%s: packs %d, wanted %d", tag, (int)got, (int)want);
    CHECK(B.vW == vW, "%s: the full table was touched", tag);
    if (!got) { CHECK(B.vW16.empty() && B.wRef == 0, "%s: a table without the flag", tag); return; }
    for (int32_t lv = 0; lv < B.capV; ++lv)
        for (int e = 0; e < 8; ++e) {
            const int16_t off = B.vW16[(size_t)lv * 8 + e];
            if (e >= (int)B.vCount[lv]) { CHECK(off == 0, "%s: padded entry", tag); continue; }
            CHECK(bitsOf(fusedWeightFromOffset(B.wRef, off)) == bitsOf(vW[(size_t)e * B.capV + lv]), "%s: vertex %d weight %d", tag, lv, e);
        }
}

int main() {
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const int32_t pt[6] = {0, 0, 0, 0, 0, 0};
    { HostMesh m = makeBox(13, 7, 5, 0, 5, lo, hi, pt); qualifies("box 13x7x5", m, true); }
    { HostMesh m = makeBox(50, 50, 50, 0, 50, lo, hi, pt); qualifies("box 50x50x50", m, true); }
    { HostMesh m = makeBox(100, 20, 20, 0, 20, lo, hi, pt); qualifies("box 100x20x20", m, true); }
    { HostMesh m = makeBox(12, 6, 12, 3, 9, lo, hi, pt); qualifies("slab 3..9 of a 12x6x12 box", m, true); }
    {   // the rule, on weight sets written by hand
        const int64_t eighth = bitsOf(0.125);
        { FusedBlocks B = handMade(8, eighth + 1000, 65535); checkHandMade("spread 65535", B, true); }
        { FusedBlocks B = handMade(8, eighth + 1000, 65536); checkHandMade("spread 65536", B, false); }
        {   // 0.125 is a power of two: below it the exponent is one less and the doubles lie twice as close, the patterns still count on
            FusedBlocks B = handMade(8, eighth - 300, 600);
            CHECK(std::ilogb(B.vW[0]) == -4 && B.vW[0] < 0.125 && B.vW[(size_t)7 * B.capV + 15] > 0.125, "the set does not straddle 0.125");
            checkHandMade("straddling 0.125", B, true);
        }
        { FusedBlocks B = handMade(8, eighth - 40000, 65535); checkHandMade("spread 65535 across 0.125", B, true); }
        { FusedBlocks B = handMade(8, eighth, 0); checkHandMade("every weight 0.125", B, true); CHECK(B.wRef == eighth, "reference of equal weights"); }
        { FusedBlocks B = handMade(12, eighth, 10); checkHandMade("capPE 12", B, false); }
        { FusedBlocks B = handMade(6, eighth, 10); checkHandMade("capPE 6", B, false); }
        {   // a vertex of count 0 (a patch point) carries no weight: what its slots hold does not count
            FusedBlocks B = handMade(8, eighth, 100);
            B.vCount[3] = 0;
            for (int e = 0; e < 8; ++e) B.vW[(size_t)e * B.capV + 3] = 1e30;
            checkHandMade("a patch point with stale slots", B, true);
        }
        {   // a short vertex: its slots beyond the count do not count either, and come out 0
            FusedBlocks B = handMade(8, eighth, 100);
            B.vCount[5] = 4;
            for (int e = 4; e < 8; ++e) B.vW[(size_t)e * B.capV + 5] = 0.0;
            checkHandMade("a vertex of four cells", B, true);
        }
        { FusedBlocks B = handMade(8, eighth, 100); B.vW[(size_t)2 * B.capV + 7] = -0.125; checkHandMade("a negative weight", B, false); }
    }
    {   // the jittered mesh of fused_blocks_test.cpp
        HostMesh m = makeBox(11, 9, 7, 0, 7, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        splitQuads(m, 3);
        splitEdges(m, 5);
        m.computeGeometry();
        doesNotQualify("jittered 11x9x7, quads and edges split", m);
    }
    {   // hexahedra only, jittered: capPE is 8, the spread is what rules it out
        HostMesh m = makeBox(24, 16, 16, 0, 16, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        m.computeGeometry();
        doesNotQualify("jittered 24x16x16", m);
    }
    {   // a box graded 2:1 along x (the last cell twice as long as the first, geometric)
        const int nx = 20;
        HostMesh m = makeBox(nx, 8, 8, 0, 8, lo, hi, pt);
        const double r = std::pow(2.0, 1.0 / (nx - 1));
        for (int32_t p = 0; p < m.nPoints; ++p) {
            const double i = m.points[3 * (size_t)p] * nx;
            m.points[3 * (size_t)p] = (std::pow(r, i) - 1.0) / (std::pow(r, (double)nx) - 1.0);
        }
        m.computeGeometry();
        doesNotQualify("box 20x8x8 graded 2:1 along x", m);
    }
    {   // the switch: a mesh that packs keeps the full table alone
        HostMesh m = makeBox(13, 7, 5, 0, 5, lo, hi, pt);
        if (m.magSf.empty()) m.computeGeometry();
        m.computeDerived();
        const StaticData s = buildStaticData(m);
        setenv("QGD_FUSED_PACKED_W", "0", 1);
        const FusedBlocks B = buildFusedBlocks(s, false);
        unsetenv("QGD_FUSED_PACKED_W");
        CHECK(B.packedW == 0 && B.vW16.empty() && B.vW.size() == (size_t)B.nBlocks * B.capPE * B.capV, "QGD_FUSED_PACKED_W=0 packs");
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
