// The host side of the fused step: qgd_setup.cpp buildFusedBlocks (CPU only; compiled by tests/test_fused_blocks_host.py with plain g++ from the
// library's own host sources).  Checks the tables the kernel trusts blindly:
//   * every owned cell is an own cell of exactly one block, ghost cells of none; every cell a neighbouring shard waits for sits in one of
//     the first nLayerBlocks blocks (whole bricks: they hold other cells too), and every one of those blocks holds such a cell;
//   * a block's face list holds every internal face of its own cells, once, with owner / neighbour / vertex positions that point at those very
//     labels; every list is padded to its stride with its last entry;
//   * the face entries of an own cell are the cell's faces in ascending label with the right side bit, patch faces as ~label;
//   * a vertex's cell positions are its pointCells in order, with the weights of the vertex kernel's table; patch points have count 0;
//   * the maxima are the maxima, and no block of more than 32 cells needs more LDS than lets three blocks share a CU;
//   * blocks that share a template have the same tables: the builder compares them once and counts the blocks whose fingerprint matched
//     a template that their tables did not (FusedBlocks::templateMismatches; each gets a template of its own).  With the full fingerprint
//     the count is zero and the template counts are what they were before the comparison existed.  Compiled a second time with
//     -DQGD_TEST_TOPOHASH_BITS=1 -- a fingerprint of one bit: unlike blocks are certain to share one -- the count must be positive, and
//     every block's tables, read through its template, must still be what the mesh dictates (the entry-by-entry checks above);
//   * the launch plan (planFusedLaunch): the device takes the brick meshes' tables as they are and the thin meshes' only when told to take
//     any blocks, with the dynamic LDS this program rounds from its own maxima; refuses every table one byte below its need and with any
//     cap exceeded, whoever asks;
//   * thin meshes, whose blocks are small, have more blocks than 64-face tiles of internal faces -- the premise of
//     tests/test_courant_small_blocks_gpu.py: under Courant-number control a block needs a partial slot that is neither a face tile's
//     nor the patch kernel's.
// With arguments the program checks meshes it is handed instead of its own: "file capPE minBlocks shardOf" per mesh -- a primitives file written
// by tests/unstructured.py (tetrahedra, prisms, prisms + hexahedra: vertices of 24 / 12 cells, cells of 4 / 5 faces), the vertex stride
// wanted (the longest point -> cells row), the least number of blocks, and, when shardOf > 0, "Morton-renumber, cut into shardOf cell
// ranges, check the middle one".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <stdexcept>
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

static int mismatchesSeen = 0;

// wantTemplates: the template count of the full fingerprint, as it was before the builder compared tables (-1: not pinned)
// wantUse: 1 = the device takes these tables as they are (the brick meshes), 0 = only when told to take any blocks (the thin meshes), -1: not pinned
static FusedBlocks checkMesh(const char* tag, HostMesh& m, double minMeanCells = 0.0, int maxTemplates = -1, int wantTemplates = -1, int wantUse = -1) {
    if (m.magSf.empty()) m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    const FusedBlocks B = buildFusedBlocks(s);
    std::printf("%s: %d cells, %d blocks (%d boundary-layer), strides %d %d %d %d %d, faces computed %lld of %d\n", tag, s.nC, B.nBlocks, B.nLayerBlocks, B.capC,
                B.capV, B.capF, B.capE, B.capPE, (long long)B.facesComputed, s.nIF);
    CHECK(B.nBlocks > 0, "%s: no blocks", tag);
    if (B.nBlocks == 0) return B;
    {
        int64_t owned = 0;
        for (int32_t c = 0; c < s.nC; ++c) owned += (s.ghost.empty() || s.ghost[c] != 1) ? 1 : 0;
        const double mean = (double)owned / B.nBlocks;
        std::printf("    %.1f cells per block, %.2f cell records staged per cell, %.2f faces computed per cell\n", mean, (double)B.cellsStaged / owned,
                    (double)B.facesComputed / owned);
        CHECK(mean >= minMeanCells, "%s: %.1f cells per block on average, %.1f wanted", tag, mean, minMeanCells);
    }
    std::vector<int> ownerBlock((size_t)s.nC, -1);
    std::vector<int> tplUsed((size_t)std::max(B.nTemplates, 1), 0);
    std::printf("    %d templates for %d blocks (%s)\n", B.nTemplates, B.nBlocks, B.templated ? "shared" : "one per block");
    std::printf("    %d blocks matched a template by fingerprint and not by their tables\n", B.templateMismatches);
    mismatchesSeen += B.templateMismatches;
#ifndef QGD_TEST_TOPOHASH_BITS
    CHECK(maxTemplates < 0 || B.nTemplates <= maxTemplates, "%s: %d templates, at most %d wanted", tag, B.nTemplates, maxTemplates);
    CHECK(B.templateMismatches == 0, "%s: %d template mismatches with the full fingerprint", tag, B.templateMismatches);
    CHECK(wantTemplates < 0 || B.nTemplates == wantTemplates, "%s: %d templates, %d before the tables were compared", tag, B.nTemplates, wantTemplates);
#endif
    int32_t maxTot = 0, maxAll = 0, maxV = 0, maxF = 0, maxLds = 0, maxLdsImpl = 0;
    int64_t faces = 0;
    for (int32_t b = 0; b < B.nBlocks; ++b) {
        const int32_t nOwn = B.hdr[4 * b], nAll = B.hdr[4 * b + 1], nV = B.hdr[4 * b + 2], nF = B.hdr[4 * b + 3], nTot = B.hdr2[4 * b];
        CHECK(nOwn >= 1 && nOwn <= kFusedCells && nOwn <= nAll && nAll <= nTot && nTot <= B.capC && nAll <= kFusedCapC && nTot <= kFusedCapTot, "block %d counts", b);
        CHECK(nV <= B.capV && nV <= kFusedCapV && nF <= B.capF && nF <= kFusedCapF, "block %d counts", b);
        maxTot = std::max(maxTot, nTot); maxAll = std::max(maxAll, nAll); maxV = std::max(maxV, nV); maxF = std::max(maxF, nF);
        faces += nF;
        const int32_t lds = 48 * nTot + 32 * nAll + std::max(72 * nV + 24 * nAll, 40 * nF);   // the kernel's layout of this block's records
        maxLds = std::max(maxLds, lds);
        maxLdsImpl = std::max(maxLdsImpl, 48 * nTot + 32 * nAll + std::max({72 * nV + 24 * nAll, 32 * nF, 72 * nAll}));   // ... of the implicitDiffusion branch
        CHECK(lds <= kFusedLdsTarget || nOwn <= 32, "block %d needs %d B of LDS with %d own cells", b, lds, nOwn);
        const int32_t* cells = &B.cells[(size_t)b * B.capC];
        const int32_t* verts = &B.verts[(size_t)b * B.capV];
        for (int32_t i = nTot; i < B.capC; ++i) CHECK(cells[i] == cells[nTot - 1], "block %d cell padding", b);
        for (int32_t i = std::max(nV, 1); i < B.capV; ++i) CHECK(verts[i] == verts[std::max(nV, 1) - 1], "block %d vertex padding", b);
        std::set<int32_t> distinct(cells, cells + nTot);
        CHECK((int32_t)distinct.size() == nTot, "block %d lists a cell twice", b);
        bool hasLayerCell = false;
        for (int32_t j = 0; j < nOwn; ++j) {
            const int32_t c = cells[j];
            const int role = s.ghost.empty() ? 0 : s.ghost[c];
            CHECK(role != 1, "ghost cell %d owned by block %d", c, b);
            CHECK(ownerBlock[c] == -1, "cell %d owned twice", c);
            ownerBlock[c] = b;
            CHECK(role != 2 || b < B.nLayerBlocks, "cell %d (role %d) in block %d of %d boundary-layer blocks", c, role, b, B.nLayerBlocks);
            if (role == 2) hasLayerCell = true;
        }
        CHECK(hasLayerCell || b >= B.nLayerBlocks || nOwn < 1, "block %d of the %d boundary-layer blocks holds no cell a neighbour waits for", b, B.nLayerBlocks);
        // faces
        std::set<int32_t> want;
        for (int32_t j = 0; j < nOwn; ++j) {
            const int32_t c = cells[j];
            const size_t base = (size_t)s.cfSlice[c >> 6] * 64 + (c & 63);
            for (int i = 0; i < s.cfCount[c]; ++i) {
                const int32_t it = s.cfItem[base + (size_t)i * 64], f = it >= 0 ? it : ~it;
                if (f < s.nIF) want.insert(f);
            }
        }
        CHECK((int32_t)want.size() == nF, "block %d: %d faces listed, %d wanted", b, nF, (int)want.size());
        // the block's local topology sits in its template (hdr2[1]); blocks that share one must expand to their own labels all the same
        const int32_t tpl = B.hdr2[4 * b + 1];
        CHECK(tpl >= 0 && tpl < B.nTemplates && (B.templated || tpl == b) &&
              (B.templateMismatches > 0 || B.templated == (B.nTemplates < B.nBlocks)), "block %d template %d of %d", b, tpl, B.nTemplates);
        tplUsed[tpl]++;
        const int32_t* face = &B.faceLabel[(size_t)b * B.capF];
        const uint32_t* fpos = &B.facePos[(size_t)tpl * B.capF * 3];
        for (int32_t lf = 0; lf < nF; ++lf) {
            const int32_t f = face[lf];
            const uint32_t lc = fpos[3 * lf], va = fpos[3 * lf + 1], vb = fpos[3 * lf + 2];
            CHECK(want.count(f) == 1, "block %d lists face %d", b, f);
            CHECK((int32_t)(lc & 0xffff) < nAll && (int32_t)(lc >> 16) < nAll, "block %d face %d cell positions", b, f);
            CHECK(cells[lc & 0xffff] == s.own[f] && cells[lc >> 16] == s.nei[f], "block %d face %d owner / neighbour", b, f);
            const uint32_t pv[4] = {va & 0xffff, va >> 16, vb & 0xffff, vb >> 16};
            for (int q = 0; q < 4; ++q) {
                const int32_t v = s.verts[4 * (size_t)f + q];
                if (v >= 0) CHECK((int32_t)pv[q] < nV && verts[pv[q]] == v, "block %d face %d vertex %d", b, f, q);
            }
            if (lf > 0) CHECK(face[lf - 1] < f, "block %d faces not ascending", b);
        }
        for (int32_t lf = nF; lf < B.capF; ++lf) {
            CHECK(nF == 0 || face[lf] == face[nF - 1], "block %d face padding", b);
            for (int q = 0; q < 3; ++q) CHECK(nF == 0 || fpos[3 * lf + q] == fpos[3 * (nF - 1) + q], "block %d face padding", b);
        }
        // face entries of the own cells
        for (int32_t j = 0; j < kFusedCells; ++j) {
            const int nE = B.nEntry[(size_t)b * kFusedCells + j];
            if (j >= nOwn) { CHECK(nE == 0, "block %d entry count beyond the own cells", b); continue; }
            const int32_t c = cells[j];
            CHECK(nE == s.cfCount[c] && nE <= B.capE, "block %d cell %d entry count", b, c);
            const size_t base = (size_t)s.cfSlice[c >> 6] * 64 + (c & 63);
            for (int e = 0; e < nE; ++e) {
                const int32_t it = s.cfItem[base + (size_t)e * 64], f = it >= 0 ? it : ~it;
                const int32_t got = B.entry[((size_t)tpl * B.capE + e) * kFusedCells + j];
                if (f >= s.nIF) CHECK(got == ~f && it >= 0, "block %d cell %d patch-face entry", b, c);
                else CHECK(got >= 0 && (got >> 1) < nF && face[got >> 1] == f && (got & 1) == (it < 0 ? 1 : 0), "block %d cell %d entry %d", b, c, e);
            }
        }
        // vertex tables
        for (int32_t lv = 0; lv < B.capV; ++lv) {
            const int n = B.vCount[(size_t)b * B.capV + lv];
            if (lv >= nV) { CHECK(n == 0, "block %d vertex count beyond the list", b); continue; }
            const int32_t v = verts[lv];
            CHECK(n == s.pcCount[v] && n <= B.capPE, "block %d vertex %d count", b, v);
            const size_t base = (size_t)s.pcSlice[v >> 6] * 64 + (v & 63);
            for (int e = 0; e < n; ++e) {
                const int32_t pos = B.vPos[((size_t)tpl * B.capPE + e) * B.capV + lv];
                CHECK(pos < nTot && cells[pos] == s.pcCell[base + (size_t)e * 64], "block %d vertex %d cell %d", b, v, e);
                CHECK(B.vW[((size_t)b * B.capPE + e) * B.capV + lv] == s.pcW[base + (size_t)e * 64], "block %d vertex %d weight %d", b, v, e);
            }
        }
    }
    for (int32_t c = 0; c < s.nC; ++c) {
        const int role = s.ghost.empty() ? 0 : s.ghost[c];
        CHECK((ownerBlock[c] >= 0) == (role != 1), "cell %d (role %d) block %d", c, role, ownerBlock[c]);
    }
    for (int32_t t = 0; t < B.nTemplates; ++t) CHECK(tplUsed[t] >= 1, "%s: template %d is nobody's", tag, t);
    CHECK(maxTot == B.maxTot && maxAll == B.maxAll && maxV == B.maxV && maxF == B.maxF, "%s: maxima %d %d %d %d vs %d %d %d %d", tag, maxTot, maxAll, maxV,
          maxF, B.maxTot, B.maxAll, B.maxV, B.maxF);
    CHECK(maxLds == B.maxLds, "%s: LDS %d vs %d", tag, maxLds, B.maxLds);
    CHECK(faces == B.facesComputed && faces >= 0, "%s: faces computed", tag);
    {   // the launch plan (planFusedLaunch): whether the device takes the tables, and the dynamic LDS of its launches
        int64_t owned = 0;
        for (int32_t c = 0; c < s.nC; ++c) owned += (s.ghost.empty() || s.ghost[c] != 1) ? 1 : 0;
        // this program's own rounding: the records of the largest block to 16 B, 6 x 128 words of parked face entries behind them, to 256 B
        const int32_t park = (maxLds + 15) / 16 * 16, need = (park + 6 * 128 * 4 + 255) / 256 * 256;
        const int64_t limit = 64 * 1024;
        const FusedLaunchPlan plain = planFusedLaunch(B, owned, limit, false), any = planFusedLaunch(B, owned, limit, true);
        std::printf("    launch plan: %d B of LDS, %s\n", any.lds, plain.use ? "used" : any.use ? "used only when any blocks are" : "refused");
        CHECK(need <= limit, "%s: %d B of LDS", tag, need);
        CHECK(any.use && any.lds == need && any.ldsCell == park / 8, "%s: plan %d %d %d, %d %d wanted", tag, (int)any.use, any.lds, any.ldsCell, need, park / 8);
        CHECK(plain.lds == any.lds && plain.ldsCell == any.ldsCell && plain.ldsImpl == any.ldsImpl && plain.ldsCellImpl == any.ldsCellImpl, "%s: the mode changes the sizes", tag);
        const int32_t parkI = (maxLdsImpl + 15) / 16 * 16, needI = (parkI + 6 * 128 * 4 + 255) / 256 * 256;
        CHECK(maxLdsImpl == B.maxLdsImpl && any.ldsImpl == (needI <= limit ? needI : 0) && any.ldsCellImpl == parkI / 8, "%s: implicit layout %d %d %d, %d %d wanted", tag,
              B.maxLdsImpl, any.ldsImpl, any.ldsCellImpl, needI, parkI / 8);
        CHECK(wantUse < 0 || plain.use == (wantUse == 1), "%s: plan says %d without being told to take any blocks", tag, (int)plain.use);
        // one byte below the need: refused, whoever asks
        CHECK(!planFusedLaunch(B, owned, need - 1, false).use && !planFusedLaunch(B, owned, need - 1, true).use, "%s: used with %d B of LDS allowed", tag, need - 1);
        CHECK(planFusedLaunch(B, owned, need, true).use, "%s: refused with exactly %d B allowed", tag, need);
        // a cap exceeded: refused in both modes
        auto refused = [&](const FusedBlocks& X) { return !planFusedLaunch(X, owned, limit, false).use && !planFusedLaunch(X, owned, limit, true).use; };
        FusedBlocks X = B;
        CHECK(!refused(X), "%s: the copy is refused", tag);
        X.maxAll = kFusedCapC + 1; CHECK(refused(X), "%s: maxAll over its cap", tag); X.maxAll = B.maxAll;
        X.maxTot = kFusedCapTot + 1; CHECK(refused(X), "%s: maxTot over its cap", tag); X.maxTot = B.maxTot;
        X.capV = kFusedCapV + 8; CHECK(refused(X), "%s: capV over its cap", tag); X.capV = B.capV;
        X.capF = kFusedCapF + 8; CHECK(refused(X), "%s: capF over its cap", tag); X.capF = B.capF;
        X.capPE = 256; CHECK(refused(X), "%s: capPE over 255", tag); X.capPE = B.capPE;
        X.nBlocks = 0; CHECK(refused(X), "%s: no blocks", tag); X.nBlocks = B.nBlocks;
        CHECK(!refused(X), "%s: the restored copy is refused", tag);
    }
    return B;
}

// A chain of cells (one internal face and four vertices of its own per cell: the 256 vertices a block stages hold 50 to 60 cells) has
// more blocks than 64-face tiles of internal faces.  Under Courant-number control the blocks once wrote their partials into slots
// [0, nBlocks) of a table whose slots [faceBlocks, faceBlocks + bfaceBlocks) belong to the patch kernel's 256-face workgroups: blocks
// faceBlocks .. nBlocks-1 then overwrote the partials of the first 256 * (nBlocks - faceBlocks) patch faces.  inletOverwritten: patch 0
// (xMin, the inlet of tests/test_courant_small_blocks_gpu.py) lies among those faces entirely.
// (No mesh of hexahedra goes past the END of that table: a cell has 6 = patchFaces + 2 * internalFaces faces, so the table holds at least
// (2 f + 6) / 256 slots per cell (f = internal faces per cell), and a block is cut only when it is over a cap of the kernel -- 128 cells, or
// 256 vertices at no more than 4 per face -- which leaves at most max(1 / 64, f / 32) blocks per cell even when every cut halves a block
// that was just over; the two meet at f > 1 only, where faces share vertices and the blocks grow again.  The chains below have
// 19 blocks against 16 + 17 slots.)
static void checkSmallBlocks(const char* tag, HostMesh& m, bool inletOverwritten) {
    const FusedBlocks B = checkMesh(tag, m, 0.0, -1, -1, 0);
    const int32_t nIF = m.nInternalFaces, nBF = m.nFaces - m.nInternalFaces;
    const int32_t faceBlocks = (nIF + 63) / 64, bfaceBlocks = (nBF + 255) / 256;
    std::printf("    %d blocks, %d face tiles, %d patch workgroups\n", B.nBlocks, faceBlocks, bfaceBlocks);
    CHECK(B.nBlocks > faceBlocks, "%s: %d blocks, %d face tiles", tag, B.nBlocks, faceBlocks);
    const int32_t inletEnd = m.patches[0].start - nIF + m.patches[0].size;
    CHECK(!inletOverwritten || (m.patches[0].size > 0 && inletEnd <= 256 * (B.nBlocks - faceBlocks)), "%s: patch 0 ends at patch face %d, blocks cover %d", tag,
          inletEnd, 256 * (B.nBlocks - faceBlocks));
}

static HostMesh readPrimitives(const char* path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error(std::string("cannot read ") + path);
    HostMesh m;
    int32_t nPatches = 0, nFacePoints = 0;
    in >> m.nPoints >> m.nFaces >> m.nInternalFaces >> m.nCells >> nPatches >> nFacePoints;
    auto read = [&](auto& v, size_t n) { v.resize(n); for (auto& x : v) in >> x; };
    read(m.points, 3 * (size_t)m.nPoints);
    read(m.faceOffsets, (size_t)m.nFaces + 1);
    read(m.facePoints, (size_t)nFacePoints);
    read(m.owner, (size_t)m.nFaces);
    read(m.neighbour, (size_t)m.nInternalFaces);
    std::vector<int32_t> start, size, type;
    read(start, (size_t)nPatches); read(size, (size_t)nPatches); read(type, (size_t)nPatches);
    if (!in) throw std::runtime_error(std::string("short file ") + path);
    for (int i = 0; i < nPatches; ++i) {
        Patch p;
        p.name = "patch" + std::to_string(i);
        p.type = type[i]; p.start = start[i]; p.size = size[i];
        m.patches.push_back(p);
    }
    const std::string err = m.check();
    if (!err.empty()) throw std::runtime_error(std::string(path) + ": " + err);
    m.computeGeometry();
    return m;
}

static int checkFiles(int argc, char** argv) {
    // per mesh: file, vertex stride capPE, least number of blocks, shards (0: the whole mesh), least and largest number of face entries of an own cell
    CHECK((argc - 1) % 6 == 0, "%d arguments: six per mesh", argc - 1);
    for (int a = 1; a + 5 < argc; a += 6) {
        const int wantPE = std::atoi(argv[a + 1]), minBlocks = std::atoi(argv[a + 2]), shardOf = std::atoi(argv[a + 3]);
        const int wantMinE = std::atoi(argv[a + 4]), wantMaxE = std::atoi(argv[a + 5]);
        HostMesh m = readPrimitives(argv[a]);
        std::string tag = argv[a];
        if (shardOf > 0) {
            const std::vector<int32_t> order = mortonOrder(m);
            renumberCells(m, order.data(), nullptr);
            std::vector<int32_t> cellStart;
            for (int r = 0; r <= shardOf; ++r) cellStart.push_back((int32_t)((int64_t)m.nCells * r / shardOf));
            m = extractShard(m, shardOf, cellStart.data(), shardOf / 2);
            tag += " (Morton order, shard " + std::to_string(shardOf / 2) + " of " + std::to_string(shardOf) + ")";
            int32_t ghosts = 0;
            for (uint8_t g : m.cellIsGhost) ghosts += g ? 1 : 0;
            std::printf("%s: %d ghost cells for %d owned\n", tag.c_str(), ghosts, m.nCells - ghosts);
            CHECK(ghosts > 0 && ghosts < m.nCells, "%s: %d ghosts of %d cells", tag.c_str(), ghosts, m.nCells);
        }
        const FusedBlocks B = checkMesh(tag.c_str(), m);
        CHECK(B.capPE == wantPE, "%s: capPE %d, %d wanted", tag.c_str(), B.capPE, wantPE);
        CHECK(B.nBlocks >= minBlocks, "%s: %d blocks, at least %d wanted", tag.c_str(), B.nBlocks, minBlocks);
        CHECK(B.templateMismatches == 0, "%s: %d template mismatches", tag.c_str(), B.templateMismatches);
        int32_t minE = 1 << 30, maxE = 0;
        for (int32_t b = 0; b < B.nBlocks; ++b)
            for (int32_t j = 0; j < B.hdr[4 * b]; ++j) {
                const int nE = B.nEntry[(size_t)b * kFusedCells + j];
                minE = std::min(minE, (int32_t)nE); maxE = std::max(maxE, (int32_t)nE);
            }
        std::printf("    face entries per own cell: %d .. %d (stride %d)\n", minE, maxE, B.capE);
        CHECK(minE == wantMinE && maxE == wantMaxE, "%s: face entries per cell %d .. %d, %d .. %d wanted", tag.c_str(), minE, maxE, wantMinE, wantMaxE);
    }
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return checkFiles(argc, argv);
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    const int32_t pt[6] = {0, 0, 0, 0, 0, 0};
    { HostMesh m = makeBox(16, 8, 8, 0, 8, lo, hi, pt); checkMesh("box 16x8x8 (bricks)", m, 0.0, -1, 8, 1); }
    { HostMesh m = makeBox(13, 7, 5, 0, 5, lo, hi, pt); checkMesh("box 13x7x5 (ragged)", m, 0.0, -1, 5, 1); }
    { HostMesh m = makeBox(3, 2, 2, 0, 2, lo, hi, pt); checkMesh("box 3x2x2", m, 0.0, -1, 1); }
    {
        HostMesh m = makeBox(11, 9, 7, 0, 7, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        splitQuads(m, 3);
        splitEdges(m, 5);
        checkMesh("jittered, every third quad split, every fifth edge split (triangles, polygons)", m, 0.0, -1, 7);
    }
    { HostMesh m = makeBox(12, 6, 12, 3, 9, lo, hi, pt); checkMesh("slab 3..9 of a 12x6x12 box (two cuts)", m, 0.0, -1, 3); }
    // what a cut must not cost: a 50-plane slab between two cuts keeps brick-shaped blocks -- 13 brick layers of 3 or 4
    // planes, 123 cells per block -- and the blocks of the planes a neighbour waits for are whole bricks, not flat one-plane ones
    { HostMesh m = makeBox(80, 80, 150, 49, 101, lo, hi, pt); checkMesh("planes 50..100 of an 80x80x150 box (50 owned planes between two ghost planes)", m, 120.0, 2600 - 8 * 18 * 11 + 40, 730, 1); }   // the 8 x 18 x 11 bricks without a patch face or a ghost plane share a handful of templates
    { HostMesh m = makeBox(50, 50, 50, 0, 50, lo, hi, pt); checkMesh("box 50x50x50 (extents 8x4x4 bricks do not divide: 5x5x5 ones)", m, 120.0, 1000 - 8 * 8 * 8 + 1, 489, 1); }   // 512 interior cubes, ONE template
    {   // a jittered, Morton-renumbered mesh: no two blocks list their cells alike -> one template per block, the kernel's untemplated path
        HostMesh m = makeBox(24, 16, 16, 0, 16, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        splitQuads(m, 7);
        checkMesh("jittered 24x16x16, every seventh quad split", m, 0.0, -1, 52); }
    {   // the thin meshes of tests/test_courant_small_blocks_gpu.py (PolyMesh.box takes the same arguments): six generic patches, three solved directions
        const double lo2[3] = {0.0, 0.45, 0.45}, hi2[3] = {7.0, 0.55, 0.55};
        { HostMesh m = makeBox(1024, 1, 1, 0, 1, lo, hi, pt); checkSmallBlocks("thin 1024x1x1", m, true); }
        { HostMesh m = makeBox(700, 1, 1, 0, 1, lo2, hi2, pt); checkSmallBlocks("thin 700x1x1, cells of 0.01 x 0.1 x 0.1", m, true); }
        { HostMesh m = makeBox(1, 1, 700, 0, 700, lo, hi, pt); checkSmallBlocks("thin 1x1x700", m, false); }
    }
#ifdef QGD_TEST_TOPOHASH_BITS
    CHECK(mismatchesSeen > 0, "a fingerprint of %d bits and no block whose tables differ from its template's", (int)QGD_TEST_TOPOHASH_BITS);
#endif
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("ok\n");
    return 0;
}
