// The per-face streams of the fused step block-major and packed (qgd_setup.cpp packFusedFaceStreams, FusedBlocks::fW16 / fKC / fwRef / fhRef;
// CPU only, compiled by tests/test_fused_packed_faces_host.py with plain g++ from the library's own host sources).
//   * uniform boxes and a slab shard QUALIFY: their vertex weights pack, the patterns of w over every computed face slot lie within 65 535 of
//     each other and those of hQGDf fall into one class per distinct axis spacing (17x9x9: two, 16x8x12: three).  Every slot, decoded
//     (reference + offset, taken as a double; kind = byte & 3), is s.w / s.hf / s.fkind of the slot's face bit for bit; padding slots are
//     zero; references, classes and tables are the same built with 1 and with 4 threads.
//   * the RULE on streams written by hand: a spread of w of exactly 65 535 packs and 65 536 does not; four classes of hf pack and five do not;
//     a class that straddles a power of two decodes exactly; a negative w or hf does not pack; weights not packed means faces not packed.
//   * the jittered meshes and the 2:1 graded box of fused_packed_weights_test.cpp do NOT pack and lose nothing.
//   * QGD_FUSED_PACKED_F=0 builds no tables on a mesh that would pack; QGD_FUSED_PACKED_W=0 implies it.
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

// every slot of the packed tables against the mesh's own streams; returns the largest |offset|
static int checkPacked(const char* tag, const StaticData& s, const FusedBlocks& B) {
    int maxOff = 0;
    int64_t slots = 0;
    const size_t n = (size_t)B.nBlocks * B.capF;
    CHECK(B.fW16.size() == n && B.fKC.size() == n, "%s: %zu words, %zu bytes for %d blocks of %d slots", tag, B.fW16.size(), B.fKC.size(), B.nBlocks, B.capF);
    if (B.fW16.size() != n || B.fKC.size() != n) return 0;
    CHECK(B.nHfClasses >= 1 && B.nHfClasses <= 4, "%s: %d classes", tag, B.nHfClasses);
    for (int q = B.nHfClasses; q < 4; ++q) CHECK(B.fhRef[q] == 0, "%s: reference %d of %d classes is set", tag, q, B.nHfClasses);
    for (int q = 1; q < B.nHfClasses; ++q) CHECK(B.fhRef[q] > B.fhRef[q - 1] && B.fhRef[q] - B.fhRef[q - 1] > 32767, "%s: classes %d and %d overlap", tag, q - 1, q);
    for (int32_t b = 0; b < B.nBlocks; ++b) {
        const int32_t nF = B.hdr[4 * b + 3];
        for (int32_t i = 0; i < B.capF; ++i) {
            const uint32_t word = B.fW16[(size_t)b * B.capF + i];
            const uint8_t kc = B.fKC[(size_t)b * B.capF + i];
            if (i >= nF) { CHECK(word == 0 && kc == 0, "%s: block %d padding slot %d holds %08x / %02x", tag, b, i, word, (unsigned)kc); continue; }
            const int32_t f = B.faceLabel[(size_t)b * B.capF + i];
            const int16_t ow = (int16_t)(word & 0xffffu), oh = (int16_t)(word >> 16);
            const int cl = kc >> 2;
            CHECK(cl < B.nHfClasses, "%s: block %d slot %d: class %d of %d", tag, b, i, cl, B.nHfClasses);
            if (cl >= B.nHfClasses) continue;
            const double w = fusedWeightFromOffset(B.fwRef, ow), h = fusedWeightFromOffset(B.fhRef[cl], oh);
            CHECK(bitsOf(w) == bitsOf(s.w[f]), "%s: block %d face %d: w %.17g decoded, %.17g in the mesh's table", tag, b, f, w, s.w[f]);
            CHECK(bitsOf(h) == bitsOf(s.hf[f]), "%s: block %d face %d: hf %.17g decoded, %.17g in the mesh's table", tag, b, f, h, s.hf[f]);
            CHECK((kc & 3) == s.fkind[f], "%s: block %d face %d: kind %d, the mesh has %d", tag, b, f, kc & 3, (int)s.fkind[f]);
            maxOff = std::max(maxOff, std::max(std::abs((int)ow), std::abs((int)oh)));
            ++slots;
        }
    }
    CHECK(slots == B.facesComputed || B.facesComputed == 0, "%s: %lld slots, %lld faces computed", tag, (long long)slots, (long long)B.facesComputed);
    std::printf("%s: %lld face slots as offsets from w %.17g, hf in %d classes, largest |offset| %d\n", tag, (long long)slots, fromBits(B.fwRef), B.nHfClasses, maxOff);
    return maxOff;
}

static void qualifies(const char* tag, HostMesh& m, int wantClasses) {
    if (m.magSf.empty()) m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    omp_set_num_threads(4);
    const FusedBlocks B = buildFusedBlocks(s);
    CHECK(B.nBlocks > 0 && B.packedW == 1, "%s: %d blocks, weights packed %d", tag, B.nBlocks, B.packedW);
    CHECK(B.packedF == 1, "%s does not pack", tag);
    if (B.packedF != 1) return;
    CHECK(wantClasses == 0 || B.nHfClasses == wantClasses, "%s: %d classes of hf, %d expected", tag, B.nHfClasses, wantClasses);
    checkPacked(tag, s, B);
    omp_set_num_threads(1);
    const FusedBlocks B1 = buildFusedBlocks(s, false);
    omp_set_num_threads(4);
    CHECK(B1.packedF == 1 && B1.fwRef == B.fwRef && B1.nHfClasses == B.nHfClasses, "%s: w reference %lld with one thread, %lld with four", tag, (long long)B1.fwRef, (long long)B.fwRef);
    for (int q = 0; q < 4; ++q) CHECK(B1.fhRef[q] == B.fhRef[q], "%s: hf reference %d: %lld with one thread, %lld with four", tag, q, (long long)B1.fhRef[q], (long long)B.fhRef[q]);
    CHECK(B1.fW16 == B.fW16 && B1.fKC == B.fKC, "%s: the tables differ between one thread and four", tag);
}

static void doesNotQualify(const char* tag, HostMesh& m) {
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    const RawVec<double> w = s.w, hf = s.hf;
    const RawVec<uint8_t> kind = s.fkind;
    const FusedBlocks B = buildFusedBlocks(s);
    CHECK(B.nBlocks > 0, "%s: no blocks", tag);
    CHECK(B.packedF == 0 && B.fW16.empty() && B.fKC.empty() && B.fwRef == 0 && B.nHfClasses == 0, "%s packs", tag);
    for (int q = 0; q < 4; ++q) CHECK(B.fhRef[q] == 0, "%s: a reference without the flag", tag);
    CHECK(s.w == w && s.hf == hf && s.fkind == kind && !s.w.empty(), "%s: the mesh's streams were touched", tag);
    CHECK(B.faceLabel.size() == (size_t)B.nBlocks * B.capF, "%s: the face labels are gone", tag);
    std::printf("%s: not packed, streams kept\n", tag);
}

// one block of nF faces (labels 0 .. nF - 1 in slot order, capF = nF rounded up to 8) over streams given as bit patterns
struct Hand {
    StaticData s;
    FusedBlocks B;
};
static Hand handMade(const std::vector<int64_t>& w, const std::vector<int64_t>& hf) {
    Hand h;
    const int32_t nF = (int32_t)w.size();
    h.s.nF = h.s.nIF = nF;
    h.s.w.resize(nF); h.s.hf.resize(nF); h.s.fkind.resize(nF);
    for (int32_t f = 0; f < nF; ++f) { h.s.w[f] = fromBits(w[f]); h.s.hf[f] = fromBits(hf[f]); h.s.fkind[f] = (uint8_t)(f % 3 == 2 ? FK_TRI : FK_QUAD); }
    h.B.nBlocks = 1; h.B.capF = (nF + 7) / 8 * 8; h.B.packedW = 1;
    h.B.hdr.assign(4, 0); h.B.hdr[3] = nF;
    h.B.faceLabel.resize((size_t)h.B.capF);
    for (int32_t i = 0; i < h.B.capF; ++i) h.B.faceLabel[i] = std::min(i, nF - 1);
    return h;
}
// nF patterns lo .. lo + spread, both ends present
static std::vector<int64_t> ramp(int nF, int64_t lo, int64_t spread) {
    std::vector<int64_t> v(nF);
    for (int i = 0; i < nF; ++i) v[i] = i == 0 ? lo : (i == nF - 1 ? lo + spread : lo + (spread * i) / nF);
    return v;
}
static void checkHandMade(const char* tag, Hand& h, bool want, int wantClasses = 0) {
    const bool got = packFusedFaceStreams(h.B, h.s);
    CHECK(got == want && (h.B.packedF == 1) == want, "%s: packs %d, wanted %d", tag, (int)got, (int)want);
    if (!got) { CHECK(h.B.fW16.empty() && h.B.fKC.empty() && h.B.fwRef == 0 && h.B.nHfClasses == 0, "%s: a table without the flag", tag); return; }
    CHECK(wantClasses == 0 || h.B.nHfClasses == wantClasses, "%s: %d classes, %d expected", tag, h.B.nHfClasses, wantClasses);
    checkPacked(tag, h.s, h.B);
}

int main() {
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const int32_t pt[6] = {0, 0, 0, 0, 0, 0};
    { HostMesh m = makeBox(13, 7, 5, 0, 5, lo, hi, pt); qualifies("box 13x7x5", m, 0); }
    { HostMesh m = makeBox(17, 9, 9, 0, 9, lo, hi, pt); qualifies("box 17x9x9", m, 2); }
    { HostMesh m = makeBox(16, 8, 12, 0, 12, lo, hi, pt); qualifies("box 16x8x12", m, 3); }
    { HostMesh m = makeBox(50, 50, 50, 0, 50, lo, hi, pt); qualifies("box 50x50x50", m, 1); }
    { HostMesh m = makeBox(100, 20, 20, 0, 20, lo, hi, pt); qualifies("box 100x20x20", m, 0); }
    { HostMesh m = makeBox(12, 6, 12, 3, 9, lo, hi, pt); qualifies("slab 3..9 of a 12x6x12 box", m, 0); }
    {   // the rule, on streams written by hand
        const int64_t half = bitsOf(0.5), h0 = bitsOf(0.01);
        const int nF = 21;
        const std::vector<int64_t> hOne(nF, h0);
        { Hand h = handMade(ramp(nF, half + 1000, 65535), hOne); checkHandMade("w spread 65535", h, true, 1); }
        { Hand h = handMade(ramp(nF, half + 1000, 65536), hOne); checkHandMade("w spread 65536", h, false); }
        {   // 0.5 is a power of two: below it the exponent is one less and the doubles lie twice as close, the patterns still count on
            Hand h = handMade(ramp(nF, half - 300, 600), hOne);
            CHECK(h.s.w[0] < 0.5 && std::ilogb(h.s.w[0]) == -2 && h.s.w[nF - 1] > 0.5, "the set does not straddle 0.5");
            checkHandMade("w straddling 0.5", h, true, 1);
        }
        { Hand h = handMade(ramp(nF, half - 40000, 65535), hOne); checkHandMade("w spread 65535 across 0.5", h, true, 1); }
        { Hand h = handMade(std::vector<int64_t>(nF, half), hOne); checkHandMade("every w 0.5", h, true, 1); CHECK(h.B.fwRef == half && h.B.fhRef[0] == h0, "references of equal values"); }
        {   // classes of hf: k narrow clusters far apart
            auto clusters = [&](int k, int64_t width) {
                std::vector<int64_t> v(nF);
                for (int i = 0; i < nF; ++i) v[i] = h0 + (int64_t)(i % k) * 1000000 + (i / k == 0 ? 0 : (i / k == 1 ? width : (width * (i / k)) / (nF / k + 1)));
                return v;
            };
            { Hand h = handMade(ramp(nF, half, 10), clusters(4, 65535)); checkHandMade("four classes of hf, each 65535 wide", h, true, 4); }
            { Hand h = handMade(ramp(nF, half, 10), clusters(5, 100)); checkHandMade("five classes of hf", h, false); }
            { Hand h = handMade(ramp(nF, half, 10), clusters(3, 448)); checkHandMade("three classes of hf", h, true, 3); }
            // one cluster of width 65536: the greedy cut makes two classes of it (the last pattern alone), and that packs
            { Hand h = handMade(ramp(nF, half, 10), ramp(nF, h0, 65536)); checkHandMade("hf spread 65536", h, true, 2); }
            {   // a class that straddles a power of two (1/64)
                const int64_t p = bitsOf(0.015625);
                Hand h = handMade(ramp(nF, half, 10), ramp(nF, p - 500, 1000));
                CHECK(h.s.hf[0] < 0.015625 && std::ilogb(h.s.hf[0]) == -7 && h.s.hf[nF - 1] > 0.015625, "the class does not straddle 1/64");
                checkHandMade("hf straddling 1/64", h, true, 1);
            }
        }
        { Hand h = handMade(ramp(nF, half, 10), hOne); h.s.w[7] = -0.5; checkHandMade("a negative w", h, false); }
        { Hand h = handMade(ramp(nF, half, 10), hOne); h.s.hf[11] = -0.01; checkHandMade("a negative hf", h, false); }
        { Hand h = handMade(ramp(nF, half, 10), hOne); h.B.packedW = 0; checkHandMade("weights not packed", h, false); }
        {   // only the computed slots count: what a face beyond every block's count holds is not looked at
            Hand h = handMade(ramp(nF, half, 10), hOne);
            h.B.hdr[3] = nF - 1;
            h.s.w[nF - 1] = -7.0; h.s.hf[nF - 1] = 1e30;
            checkHandMade("a face no block computes", h, true, 1);
        }
    }
    {   // the jittered mesh of fused_blocks_test.cpp
        HostMesh m = makeBox(11, 9, 7, 0, 7, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        splitQuads(m, 3);
        splitEdges(m, 5);
        m.computeGeometry();
        doesNotQualify("jittered 11x9x7, quads and edges split", m);
    }
    {   // hexahedra only, jittered
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
    {   // the switches: a mesh that packs builds no face tables
        HostMesh m = makeBox(13, 7, 5, 0, 5, lo, hi, pt);
        if (m.magSf.empty()) m.computeGeometry();
        m.computeDerived();
        const StaticData s = buildStaticData(m);
        setenv("QGD_FUSED_PACKED_F", "0", 1);
        const FusedBlocks B = buildFusedBlocks(s, false);
        unsetenv("QGD_FUSED_PACKED_F");
        CHECK(B.packedW == 1 && B.packedF == 0 && B.fW16.empty() && B.fKC.empty() && B.fwRef == 0, "QGD_FUSED_PACKED_F=0 packs");
        setenv("QGD_FUSED_PACKED_W", "0", 1);
        const FusedBlocks Bw = buildFusedBlocks(s, false);
        unsetenv("QGD_FUSED_PACKED_W");
        CHECK(Bw.packedW == 0 && Bw.packedF == 0 && Bw.fW16.empty() && Bw.fKC.empty(), "QGD_FUSED_PACKED_W=0 leaves the faces packed");
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
