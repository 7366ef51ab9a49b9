// The geometry of the fused step block-major and packed (qgd_setup.cpp packFusedGeometry, FusedBlocks::gCode / gOwn / gDict / gvRef / ghRef;
// CPU only, compiled by tests/test_fused_packed_geometry_host.py with plain g++ from the library's own host sources).
//   * uniform boxes, a slab shard and the thin slab 400x400x400:0-12 QUALIFY: levels 1 and 2 apply, no block needs a 17th dictionary entry on an
//     axis, V and hQGD of the own cells span at most 65 535 patterns each.  Every slot of every block, decoded as the kernel does it
//     (dictionary[axis][code >> 12] + (code & 4095); reference + sign-extended half word), is s.Cc / s.X / s.V / s.hQGD bit for bit; slots
//     beyond a block's counts are zero; the tables are the same built with 1 and with 16 threads.
//   * the RULE on tables written by hand: 16 entries on an axis pack and 17 do not; an offset of 4 095 stays in its entry and 4 096 opens the
//     next; negative coordinates and zero decode exactly; a span of V of 65 535 packs and 65 536 does not; face streams not packed means
//     geometry not packed.
//   * jittered meshes and the 2:1 graded box do NOT pack and lose nothing; QGD_FUSED_PACKED_G=0 builds no tables on a mesh that would pack.
//   * recipes given as arguments (tests/packed_geometry_recipes.py: tag|nx,ny,nz|amplitude|seed|minOffset|minDict): the jittered box must pack at
//     every level with a largest offset >= minOffset and a largest dictionary >= minDict.
#include <omp.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

// every slot of the packed tables against the mesh's own arrays
static void checkPacked(const char* tag, const StaticData& s, const FusedBlocks& B) {
    const size_t nB = (size_t)B.nBlocks;
    CHECK(B.gCode.size() == nB * 2048 && B.gOwn.size() == nB * 128 && B.gDict.size() == nB * 96, "%s: %zu codes, %zu words, %zu patterns for %d blocks", tag,
          B.gCode.size(), B.gOwn.size(), B.gDict.size(), B.nBlocks);
    if (B.gCode.size() != nB * 2048 || B.gOwn.size() != nB * 128 || B.gDict.size() != nB * 96) return;
    int64_t slots = 0;
    int maxOff = 0, maxDict = 0;
    for (size_t b = 0; b < nB; ++b) {
        const int32_t nOwn = B.hdr[4 * b], n[2] = {B.hdr[4 * b + 1], B.hdr[4 * b + 2]};
        const uint16_t* code = &B.gCode[b * 2048];
        const int64_t* dict = &B.gDict[b * 96];
        for (int32_t j = 0; j < 128; ++j) {
            const uint32_t word = B.gOwn[b * 128 + j];
            if (j >= nOwn) { CHECK(word == 0, "%s: block %zu own slot %d beyond %d cells holds %08x", tag, b, j, nOwn, word); continue; }
            const int32_t ci = B.cells[b * B.capC + j];
            const double V = fusedWeightFromOffset(B.gvRef, (int16_t)(word & 0xffffu)), h = fusedWeightFromOffset(B.ghRef, (int16_t)(word >> 16));
            CHECK(bitsOf(V) == bitsOf(s.V[ci]), "%s: block %zu cell %d: V %.17g decoded, %.17g in the mesh", tag, b, ci, V, s.V[ci]);
            CHECK(bitsOf(h) == bitsOf(s.hQGD[ci]), "%s: block %zu cell %d: hQGD %.17g decoded, %.17g in the mesh", tag, b, ci, h, s.hQGD[ci]);
        }
        for (int set = 0; set < 2; ++set) {
            const int32_t* label = set == 0 ? &B.cells[b * B.capC] : &B.verts[b * B.capV];
            const double* src = set == 0 ? s.Cc.data() : s.X.data();
            for (int a = 0; a < 3; ++a) {   // ascending entries more than 4 095 apart, zero behind the last
                const int64_t* d = dict + set * 48 + a * 16;
                int nE = n[set] > 0 ? 16 : 0;
                while (nE > 1 && d[nE - 1] == 0) --nE;
                for (int e = 1; e < nE; ++e) CHECK(d[e] - d[e - 1] > 4095, "%s: block %zu set %d axis %d: entries %d and %d overlap", tag, b, set, a, e - 1, e);
                maxDict = std::max(maxDict, nE);
            }
            // (the kernel's slots: thread t of 256 holds slot t + 256 k as half word k -- centres -- or 4 + k -- vertices -- of its 16 bytes)
            for (int32_t q = 0; q < (set == 0 ? 1024 : 768); ++q) {
                const uint16_t c = code[(size_t)(q & 255) * 8 + set * 4 + (q >> 8)];
                if (q >= 3 * n[set]) { CHECK(c == 0, "%s: block %zu set %d slot %d beyond %d records holds %04x", tag, b, set, q, n[set], (unsigned)c); continue; }
                const int32_t r = q / 3, a = q % 3;
                const double x = fusedCoordFromCode(dict + set * 48 + a * 16, c), want = src[3 * (size_t)label[r] + a];
                CHECK(bitsOf(x) == bitsOf(want), "%s: block %zu set %d record %d axis %d: %.17g decoded, %.17g in the mesh", tag, b, set, r, a, x, want);
                maxOff = std::max(maxOff, (int)(c & 4095));
                ++slots;
            }
            for (int t = 0; t < 256; ++t) CHECK(code[(size_t)t * 8 + 7] == 0, "%s: block %zu thread %d: the spare half word is set", tag, b, t);
        }
    }
    CHECK(maxOff == B.maxGeoOffset && maxDict == B.maxGeoDict, "%s: offset %d / dictionary %d found, %d / %d reported", tag, maxOff, maxDict, B.maxGeoOffset, B.maxGeoDict);
    std::printf("%s: %lld coordinate slots in %d blocks, largest dictionary %d, largest offset %d; V from %.17g, hQGD from %.17g\n", tag, (long long)slots, B.nBlocks,
                maxDict, maxOff, fromBits(B.gvRef), fromBits(B.ghRef));
}

static FusedBlocks qualifies(const char* tag, HostMesh& m) {
    if (m.magSf.empty()) m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    omp_set_num_threads(16);
    FusedBlocks B = buildFusedBlocks(s);
    CHECK(B.nBlocks > 0 && B.packedW == 1 && B.packedF == 1, "%s: %d blocks, weights packed %d, faces %d", tag, B.nBlocks, B.packedW, B.packedF);
    CHECK(B.packedG == 1, "%s does not pack", tag);
    if (B.packedG != 1) return B;
    checkPacked(tag, s, B);
    omp_set_num_threads(1);
    const FusedBlocks B1 = buildFusedBlocks(s, false);
    omp_set_num_threads(4);
    CHECK(B1.packedG == 1 && B1.gvRef == B.gvRef && B1.ghRef == B.ghRef && B1.maxGeoDict == B.maxGeoDict && B1.maxGeoOffset == B.maxGeoOffset,
          "%s: references or maxima differ between one thread and sixteen", tag);
    CHECK(B1.gCode == B.gCode && B1.gOwn == B.gOwn && B1.gDict == B.gDict, "%s: the tables differ between one thread and sixteen", tag);
    return B;
}

static void doesNotQualify(const char* tag, HostMesh& m) {
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    const auto Cc = s.Cc;
    const auto X = s.X;
    const auto V = s.V;
    const auto hQGD = s.hQGD;
    const FusedBlocks B = buildFusedBlocks(s);
    CHECK(B.nBlocks > 0, "%s: no blocks", tag);
    CHECK(B.packedG == 0 && B.gCode.empty() && B.gOwn.empty() && B.gDict.empty() && B.gvRef == 0 && B.ghRef == 0 && B.maxGeoDict == 0 && B.maxGeoOffset == 0, "%s packs", tag);
    CHECK(s.Cc == Cc && s.X == X && s.V == V && s.hQGD == hQGD && !s.Cc.empty(), "%s: the mesh's arrays were touched", tag);
    std::printf("%s: not packed, arrays kept\n", tag);
}

// one block of n own cells (labels 0 .. n - 1, no cell across a face) and n vertices over coordinates given as bit patterns: the x of cell /
// vertex r is xs[r], y and z are 1.0; V and hQGD as given
struct Hand {
    StaticData s;
    FusedBlocks B;
};
static Hand handMade(const std::vector<int64_t>& xs, const std::vector<int64_t>& V, const std::vector<int64_t>& hq) {
    Hand h;
    const int32_t n = (int32_t)xs.size();
    h.s.nC = h.s.nP = n;
    h.s.Cc.resize(3 * (size_t)n); h.s.X.resize(3 * (size_t)n); h.s.V.resize(n); h.s.hQGD.resize(n);
    for (int32_t r = 0; r < n; ++r) {
        h.s.Cc[3 * r] = h.s.X[3 * r] = fromBits(xs[r]);
        h.s.Cc[3 * r + 1] = h.s.X[3 * r + 1] = h.s.Cc[3 * r + 2] = h.s.X[3 * r + 2] = 1.0;
        h.s.V[r] = fromBits(V[r % V.size()]); h.s.hQGD[r] = fromBits(hq[r % hq.size()]);
    }
    h.B.nBlocks = 1; h.B.capC = h.B.capV = (n + 7) / 8 * 8; h.B.packedW = 1; h.B.packedF = 1;
    h.B.hdr.assign(4, 0); h.B.hdr[0] = h.B.hdr[1] = h.B.hdr[2] = n;
    h.B.cells.resize((size_t)h.B.capC); h.B.verts.resize((size_t)h.B.capV);
    for (int32_t i = 0; i < h.B.capC; ++i) h.B.cells[i] = h.B.verts[i] = std::min(i, n - 1);
    return h;
}
static void checkHandMade(const char* tag, Hand& h, bool want, int wantDict = 0) {
    const bool got = packFusedGeometry(h.B, h.s);
    CHECK(got == want && (h.B.packedG == 1) == want, "%s: packs %d, wanted %d", tag, (int)got, (int)want);
    if (!got) { CHECK(h.B.gCode.empty() && h.B.gOwn.empty() && h.B.gDict.empty() && h.B.gvRef == 0 && h.B.ghRef == 0, "%s: a table without the flag", tag); return; }
    CHECK(wantDict == 0 || h.B.maxGeoDict == wantDict, "%s: largest dictionary %d, %d expected", tag, h.B.maxGeoDict, wantDict);
    checkPacked(tag, h.s, h.B);
}

// tag|nx,ny,nz|amplitude|seed|minOffset|minDict
static void recipe(const std::string& arg, const double* lo, const double* hi, const int32_t* pt) {
    char tag[128];
    int nx, ny, nz, minOff, minDict;
    double amp;
    unsigned long long seed;
    if (std::sscanf(arg.c_str(), "%127[^|]|%d,%d,%d|%lf|%llu|%d|%d", tag, &nx, &ny, &nz, &amp, &seed, &minOff, &minDict) != 8) {
        CHECK(false, "cannot read the recipe %s", arg.c_str());
        return;
    }
    HostMesh m = makeBox(nx, ny, nz, 0, nz, lo, hi, pt);
    m.computeGeometry();
    jitterPoints(m, amp, seed);
    m.computeGeometry();
    const std::string name = std::string("recipe ") + tag;
    const FusedBlocks B = qualifies(name.c_str(), m);
    CHECK(B.maxGeoOffset >= minOff && B.maxGeoDict >= minDict, "%s: largest offset %d (wanted >= %d), largest dictionary %d (wanted >= %d)", name.c_str(), B.maxGeoOffset,
          minOff, B.maxGeoDict, minDict);
}

int main(int argc, char** argv) {
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const int32_t pt[6] = {0, 0, 0, 0, 0, 0};
    unsetenv("QGD_FUSED_PACKED_W"); unsetenv("QGD_FUSED_PACKED_F"); unsetenv("QGD_FUSED_PACKED_G");
    if (argc > 1) {
        for (int a = 1; a < argc; ++a) recipe(argv[a], lo, hi, pt);
        std::printf(fails == 0 ? "ok\n" : "%d checks FAILED\n", fails);
        return fails == 0 ? 0 : 1;
    }
    {
        const int shapes[][3] = {{17, 9, 9}, {40, 20, 20}, {16, 8, 12}, {3, 2, 2}, {9, 5, 5}, {50, 50, 50}};
        for (const auto& sh : shapes) {
            HostMesh m = makeBox(sh[0], sh[1], sh[2], 0, sh[2], lo, hi, pt);
            char tag[64];
            std::snprintf(tag, sizeof tag, "box %dx%dx%d", sh[0], sh[1], sh[2]);
            qualifies(tag, m);
        }
        HostMesh slab = makeBox(12, 6, 12, 3, 9, lo, hi, pt);
        qualifies("slab 3..9 of a 12x6x12 box", slab);
        HostMesh thin = makeBox(400, 400, 400, 0, 12, lo, hi, pt);
        qualifies("slab 0..12 of a 400x400x400 box", thin);
        for (int which = 0; which < 2; ++which) {   // the shards of the GPU test
            HostMesh g = makeBox(16, 8, 12, 0, 12, lo, hi, pt);
            g.computeGeometry();
            const int32_t cellStart[3] = {0, g.nCells / 2, g.nCells};
            HostMesh sh = extractShard(g, 2, cellStart, which);
            qualifies(which == 0 ? "shard 0 of 2 of box 16x8x12" : "shard 1 of 2 of box 16x8x12", sh);
        }
    }
    {   // box(1,1,40): no interior vertex, nothing packs from level 1 on
        HostMesh m = makeBox(1, 1, 40, 0, 40, lo, hi, pt);
        m.computeGeometry();
        doesNotQualify("box 1x1x40", m);
    }
    {   // the rule
        const int64_t one = bitsOf(1.0), v0 = bitsOf(1e-3), h0 = bitsOf(0.05);
        auto planes = [&](int n, int64_t step, int64_t last) {   // n patterns `step` apart, the last one `last` beyond its predecessor
            std::vector<int64_t> x;
            for (int i = 0; i < n; ++i) x.push_back(i == 0 ? one : x.back() + (i == n - 1 ? last : step));
            return x;
        };
        { Hand h = handMade(planes(16, 5000, 5000), {v0}, {h0}); checkHandMade("16 entries on an axis", h, true, 16); }
        { Hand h = handMade(planes(17, 5000, 5000), {v0}, {h0}); checkHandMade("a 17th entry on an axis", h, false); }
        { Hand h = handMade(planes(17, 5000, 4095), {v0}, {h0}); checkHandMade("an offset of 4 095 stays in its entry", h, true, 16); CHECK(h.B.maxGeoOffset == 4095, "largest offset %d", h.B.maxGeoOffset); }
        { Hand h = handMade(planes(17, 5000, 4096), {v0}, {h0}); checkHandMade("an offset of 4 096 opens the next entry", h, false); }
        { Hand h = handMade({bitsOf(-0.5), bitsOf(-0.5) + 77, 0, bitsOf(0.25), bitsOf(-1e-300)}, {v0}, {h0}); checkHandMade("negative coordinates and zero", h, true); }
        { Hand h = handMade(planes(4, 10, 10), {v0, v0 + 65535}, {h0}); checkHandMade("a span of V of 65 535", h, true); CHECK(h.B.maxGeoOffset <= 30, "largest offset %d", h.B.maxGeoOffset); }
        { Hand h = handMade(planes(4, 10, 10), {v0, v0 + 65536}, {h0}); checkHandMade("a span of V of 65 536", h, false); }
        { Hand h = handMade(planes(4, 10, 10), {v0}, {h0, h0 + 65536}); checkHandMade("a span of hQGD of 65 536", h, false); }
        { Hand h = handMade(planes(4, 10, 10), {v0}, {h0}); h.B.packedF = 0; checkHandMade("face streams not packed", h, false); }
    }
    {   // what does not pack keeps everything
        HostMesh m = makeBox(11, 9, 7, 0, 7, lo, hi, pt);
        m.computeGeometry();
        jitterPoints(m, 0.15, 7);
        m.computeGeometry();
        doesNotQualify("jittered box 11x9x7", m);
        HostMesh g = makeBox(20, 8, 8, 0, 8, lo, hi, pt);
        const double r = std::pow(2.0, 1.0 / 19);
        for (int32_t p = 0; p < g.nPoints; ++p) g.points[3 * (size_t)p] = (std::pow(r, g.points[3 * (size_t)p] * 20) - 1.0) / (std::pow(r, 20.0) - 1.0);
        g.computeGeometry();
        doesNotQualify("graded box 20x8x8", g);
    }
    {   // the switch
        HostMesh m = makeBox(17, 9, 9, 0, 9, lo, hi, pt);
        m.computeGeometry();
        m.computeDerived();
        const StaticData s = buildStaticData(m);
        setenv("QGD_FUSED_PACKED_G", "0", 1);
        const FusedBlocks B = buildFusedBlocks(s);
        unsetenv("QGD_FUSED_PACKED_G");
        CHECK(B.packedW == 1 && B.packedF == 1 && B.packedG == 0 && B.gCode.empty() && B.gOwn.empty() && B.gDict.empty(), "QGD_FUSED_PACKED_G=0 packs");
        setenv("QGD_FUSED_PACKED_F", "0", 1);
        const FusedBlocks B2 = buildFusedBlocks(s);
        unsetenv("QGD_FUSED_PACKED_F");
        CHECK(B2.packedW == 1 && B2.packedF == 0 && B2.packedG == 0 && B2.gCode.empty(), "QGD_FUSED_PACKED_F=0 leaves the geometry packed");
    }
    std::printf(fails == 0 ? "ok\n" : "%d checks FAILED\n", fails);
    return fails == 0 ? 0 : 1;
}
