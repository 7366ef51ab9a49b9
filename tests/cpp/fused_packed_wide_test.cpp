// The packed tables of the fused step at offsets that use all 16 bits (qgd_setup.cpp packFusedWeights / packFusedFaceStreams; CPU only, compiled
// by tests/test_fused_packed_wide_host.py with plain g++ from the library's own host sources).  A uniform box keeps every offset below 128, so a
// decode that reads the low byte alone, or never adds the offset at all, is right or nearly right on it; a box whose interior points are moved
// by ~1e-12 of the cell size still packs, and its offsets fill the half words.  Every argument is one recipe of tests/packed_wide_recipes.py,
//      tag|nx,ny,nz|hix,hiy,hiz|amplitude|seed|packedWeights|packedFaces|hfClasses
// (packedWeights = -1: a uniform box, reported and not judged), and for each the program
//   * builds the tables with 1 and with 4 threads: the same references, classes, tables and reported figures;
//   * checks the recipe's expectation: the flags, the classes, max(maxWeightOffset, maxFaceOffset) >= 16384 where anything packs and
//     maxFaceOffset >= 16384 where the faces pack;
//   * decodes every used slot (reference + offset, taken as a double; kind = byte & 3) against vW, s.w, s.hf and s.fkind bit for bit;
//   * applies WRONG decodes to the same tables -- the low byte alone, the half word zero-extended, no offset, the halves of a face word
//     swapped, the halves of a pair of weight offsets swapped, every class read as class 0, class 3 read as class 2 -- and counts the slots each
//     changes: at least 1 % of the used slots of every table it applies to, one of them by more than 4096 patterns (1e-12 relative).
#include <omp.h>

#include <algorithm>
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
            if (fails < 30) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
            ++fails;                                       \
        }                                                  \
    } while (0)

static int64_t bitsOf(double w) { int64_t b; std::memcpy(&b, &w, 8); return b; }

enum Mutant { EXACT, LOW_BYTE, ZERO_EXTENDED, NO_OFFSET, FACE_HALVES_SWAPPED, WEIGHT_PAIR_SWAPPED, CLASS_ZERO, CLASS_3_AS_2, N_MUTANTS };
static const char* const kMutantName[N_MUTANTS] = {"exact", "low byte only", "zero-extended half word", "offset taken as 0", "face half words swapped",
                                                   "weight pair halves swapped", "class forced to 0", "class 3 read as class 2"};

// a half word as the decode under test takes it: the offset added to the reference
static int64_t offsetOf(uint16_t half, Mutant mu) {
    switch (mu) {
        case LOW_BYTE: return (int8_t)(half & 0xffu);
        case ZERO_EXTENDED: return (int64_t)half;
        case NO_OFFSET: return 0;
        default: return (int16_t)half;
    }
}
static double decode(int64_t ref, uint16_t half, Mutant mu) {
    if (mu == EXACT) return fusedWeightFromOffset(ref, (int16_t)half);   // (the library's own decode: what a change to it breaks first)
    const int64_t bits = ref + offsetOf(half, mu);
    double w;
    std::memcpy(&w, &bits, 8);
    return w;
}

struct Count {
    int64_t used = 0, changed = 0, worst = 0;   // slots looked at, slots whose decoded value is not the mesh's, the largest difference in patterns
    void add(int64_t a, int64_t b) { const int64_t d = a > b ? a - b : b - a; changed += d != 0; worst = std::max(worst, d); }
};

// the vertex weights under a decode: slot e of vertex lv of block b against vW
static Count weightsUnder(const FusedBlocks& B, Mutant mu) {
    Count c;
    for (int64_t v = 0; v < (int64_t)B.nBlocks * B.capV; ++v)
        for (int e = 0; e < (int)B.vCount[v]; ++e) {
            const int from = mu == WEIGHT_PAIR_SWAPPED ? (e ^ 1) : e;
            const double w = decode(B.wRef, (uint16_t)B.vW16[(size_t)v * 8 + from], mu);
            const double want = B.vW[((size_t)(v / B.capV) * 8 + e) * (size_t)B.capV + (size_t)(v % B.capV)];
            ++c.used;
            c.add(bitsOf(w), bitsOf(want));
        }
    return c;
}
// the face slots under a decode: a slot counts once, changed where w, hf or the kind is
static Count facesUnder(const StaticData& s, const FusedBlocks& B, Mutant mu, int64_t perClass[4]) {
    Count c;
    for (int32_t b = 0; b < B.nBlocks; ++b)
        for (int32_t i = 0; i < B.hdr[4 * b + 3]; ++i) {
            const uint32_t word = B.fW16[(size_t)b * B.capF + i];
            const uint8_t kc = B.fKC[(size_t)b * B.capF + i];
            const int32_t f = B.faceLabel[(size_t)b * B.capF + i];
            uint16_t lo = (uint16_t)(word & 0xffffu), hi = (uint16_t)(word >> 16);
            if (mu == FACE_HALVES_SWAPPED) std::swap(lo, hi);
            int cl = kc >> 2;
            if (perClass) ++perClass[cl & 3];
            if (mu == CLASS_ZERO) cl = 0;
            if (mu == CLASS_3_AS_2 && cl == 3) cl = 2;
            const int64_t dw = std::llabs(bitsOf(decode(B.fwRef, lo, mu)) - bitsOf(s.w[f]));
            const int64_t dh = std::llabs(bitsOf(decode(B.fhRef[cl & 3], hi, mu)) - bitsOf(s.hf[f]));
            ++c.used;
            c.changed += dw != 0 || dh != 0 || (kc & 3) != s.fkind[f];
            c.worst = std::max(c.worst, std::max(dw, dh));
        }
    return c;
}

struct Recipe {
    std::string tag;
    int n[3] = {0, 0, 0};
    double hi[3] = {1, 1, 1};
    double amp = 0;
    unsigned long long seed = 0;
    int packedW = 0, packedF = 0, classes = 0;   // packedW = -1: a uniform box, reported only
};

static bool parse(const char* arg, Recipe& r) {
    std::vector<std::string> part(1);
    for (const char* p = arg; *p; ++p) { if (*p == '|') part.emplace_back(); else part.back() += *p; }
    if (part.size() != 8) return false;
    r.tag = part[0];
    if (std::sscanf(part[1].c_str(), "%d,%d,%d", &r.n[0], &r.n[1], &r.n[2]) != 3) return false;
    char* end = nullptr;
    const char* h = part[2].c_str();
    for (int k = 0; k < 3; ++k) { r.hi[k] = std::strtod(h, &end); if (end == h) return false; h = *end == ',' ? end + 1 : end; }
    r.amp = std::strtod(part[3].c_str(), nullptr);
    r.seed = std::strtoull(part[4].c_str(), nullptr, 10);
    r.packedW = std::atoi(part[5].c_str()); r.packedF = std::atoi(part[6].c_str()); r.classes = std::atoi(part[7].c_str());
    return r.n[0] > 0 && r.n[1] > 0 && r.n[2] > 0;
}

static void runRecipe(const Recipe& r) {
    const char* tag = r.tag.c_str();
    const bool judged = r.packedW >= 0;
    const double lo[3] = {0, 0, 0};
    const int32_t pt[6] = {0, 0, 0, 0, 0, 0};
    HostMesh m = makeBox(r.n[0], r.n[1], r.n[2], 0, r.n[2], lo, r.hi, pt);
    if (r.amp > 0) jitterPoints(m, r.amp, r.seed);
    if (m.magSf.empty()) m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    omp_set_num_threads(4);
    const FusedBlocks B = buildFusedBlocks(s);
    omp_set_num_threads(1);
    const FusedBlocks B1 = buildFusedBlocks(s);
    omp_set_num_threads(4);
    CHECK(B.nBlocks > 0, "%s: no blocks", tag);
    // one thread and four: the same decision, references, classes, tables and figures
    CHECK(B1.packedW == B.packedW && B1.wRef == B.wRef && B1.vW16 == B.vW16 && B1.maxWeightOffset == B.maxWeightOffset, "%s: the weight tables differ between one thread and four", tag);
    CHECK(B1.packedF == B.packedF && B1.fwRef == B.fwRef && B1.nHfClasses == B.nHfClasses && B1.fW16 == B.fW16 && B1.fKC == B.fKC && B1.maxFaceOffset == B.maxFaceOffset,
          "%s: the face tables differ between one thread and four", tag);
    for (int q = 0; q < 4; ++q) CHECK(B1.fhRef[q] == B.fhRef[q], "%s: hf reference %d differs between one thread and four", tag, q);

    // the offsets as the tables hold them
    int wMin = 0, wMax = 0, fwMin = 0, fwMax = 0, fhMin = 0, fhMax = 0;
    if (B.packedW)
        for (int64_t v = 0; v < (int64_t)B.nBlocks * B.capV; ++v)
            for (int e = 0; e < (int)B.vCount[v]; ++e) { const int o = B.vW16[(size_t)v * 8 + e]; wMin = std::min(wMin, o); wMax = std::max(wMax, o); }
    if (B.packedF)
        for (int32_t b = 0; b < B.nBlocks; ++b)
            for (int32_t i = 0; i < B.hdr[4 * b + 3]; ++i) {
                const uint32_t word = B.fW16[(size_t)b * B.capF + i];
                const int ow = (int16_t)(word & 0xffffu), oh = (int16_t)(word >> 16);
                fwMin = std::min(fwMin, ow); fwMax = std::max(fwMax, ow); fhMin = std::min(fhMin, oh); fhMax = std::max(fhMax, oh);
            }
    const int maxW = std::max(-wMin, wMax), maxF = std::max(std::max(-fwMin, fwMax), std::max(-fhMin, fhMax));
    CHECK(B.maxWeightOffset == maxW && B.maxFaceOffset == maxF, "%s: the builder reports %d / %d, the tables hold %d / %d", tag, B.maxWeightOffset, B.maxFaceOffset, maxW, maxF);
    int64_t perClass[4] = {0, 0, 0, 0};
    Count exactW, exactF;
    if (B.packedW) exactW = weightsUnder(B, EXACT);
    if (B.packedF) exactF = facesUnder(s, B, EXACT, perClass);
    std::printf("%s: packedWeights %d offsets [%d, %d], packedFaces %d hfClasses %d w offsets [%d, %d] hf offsets [%d, %d] slots per class %lld %lld %lld %lld\n", tag,
                B.packedW, wMin, wMax, B.packedF, B.nHfClasses, fwMin, fwMax, fhMin, fhMax, (long long)perClass[0], (long long)perClass[1], (long long)perClass[2],
                (long long)perClass[3]);
    if (judged) {
        CHECK(B.packedW == r.packedW && B.packedF == r.packedF && B.nHfClasses == r.classes, "%s: packed %d / %d in %d classes, the recipe says %d / %d in %d", tag, B.packedW,
              B.packedF, B.nHfClasses, r.packedW, r.packedF, r.classes);
        if (B.packedW) CHECK(std::max(maxW, maxF) >= 16384, "%s: the largest |offset| is %d", tag, std::max(maxW, maxF));
        if (B.packedF) CHECK(maxF >= 16384, "%s: the largest |offset| of a face word is %d", tag, maxF);
    } else {
        CHECK(B.packedW == 1 && B.packedF == 1, "%s: a uniform box does not pack", tag);
    }
    // the decode itself: every used slot is the mesh's value bit for bit
    if (B.packedW) CHECK(exactW.used > 0 && exactW.changed == 0, "%s: %lld of %lld weights decode to another value", tag, (long long)exactW.changed, (long long)exactW.used);
    if (B.packedF) {
        CHECK(exactF.used == B.facesComputed && exactF.changed == 0, "%s: %lld of %lld face slots decode to other values", tag, (long long)exactF.changed, (long long)exactF.used);
        for (int q = B.nHfClasses; q < 4; ++q) CHECK(perClass[q] == 0 && B.fhRef[q] == 0, "%s: class %d of %d is in use", tag, q, B.nHfClasses);
        for (int q = 0; q < B.nHfClasses; ++q) CHECK(perClass[q] > 0, "%s: class %d is empty", tag, q);
    }
    // the wrong decodes
    for (int k = 1; k < N_MUTANTS; ++k) {
        const Mutant mu = (Mutant)k;
        const bool onWeights = B.packedW && (mu == LOW_BYTE || mu == ZERO_EXTENDED || mu == NO_OFFSET || mu == WEIGHT_PAIR_SWAPPED);
        const bool onFaces = B.packedF && (mu == LOW_BYTE || mu == ZERO_EXTENDED || mu == NO_OFFSET || mu == FACE_HALVES_SWAPPED ||
                                           (mu == CLASS_ZERO && B.nHfClasses >= 2) || (mu == CLASS_3_AS_2 && B.nHfClasses == 4));
        if (!onWeights && !onFaces) continue;
        Count cw, cf;
        if (onWeights) cw = weightsUnder(B, mu);
        if (onFaces) cf = facesUnder(s, B, mu, nullptr);
        std::printf("%s: mutant '%s': weights %lld of %lld changed, worst %lld; faces %lld of %lld changed, worst %lld\n", tag, kMutantName[k], (long long)cw.changed,
                    (long long)cw.used, (long long)cw.worst, (long long)cf.changed, (long long)cf.used, (long long)cf.worst);
        if (!judged) continue;
        if (onWeights) CHECK(100 * cw.changed >= cw.used && cw.worst > 4096, "%s: '%s' changes %lld of %lld weights, by %lld patterns at most", tag, kMutantName[k],
                             (long long)cw.changed, (long long)cw.used, (long long)cw.worst);
        if (onFaces) CHECK(100 * cf.changed >= cf.used && cf.worst > 4096, "%s: '%s' changes %lld of %lld face slots, by %lld patterns at most", tag, kMutantName[k],
                           (long long)cf.changed, (long long)cf.used, (long long)cf.worst);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("no recipes given\n"); return 2; }
    unsetenv("QGD_FUSED_PACKED_W");
    unsetenv("QGD_FUSED_PACKED_F");
    for (int a = 1; a < argc; ++a) {
        Recipe r;
        if (!parse(argv[a], r)) { std::printf("cannot read the recipe '%s'\n", argv[a]); return 2; }
        runRecipe(r);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
