// Host set-up probe (CPU only): g++ -std=c++17 -O2 -fopenmp -I qgdsolver_amd/csrc scripts/probes/setup_harness.cpp
//     qgdsolver_amd/csrc/{qgd_mesh,qgd_partition,qgd_setup}.cpp
//   setup_harness [n=128]              the host stages of an n^3 box, timed
//   setup_harness digest MESH...       one FNV-1a digest per table of the mesh's FusedBlocks and its scalar fields, to compare two builds of
//                                      the block builder.  No digest is pinned anywhere: they depend on the compiler's floating-point
//                                      contraction in buildStaticData.  MESH is one of
//       NXxNYxNZ                       a box
//       NXxNYxNZ:Z0-Z1                 the slab of planes z0 .. z1 of it (a shard with two cuts)
//       jitter11 | jitter24 | graded   jittered 11x9x7 with quads and edges split; jittered 24x16x16; 20x8x8 graded 2:1 along x
//       FILE[:K]                       a primitives file of tests/unstructured.py; :K = Morton order, the middle one of K shards
#include "qgd_mesh.hpp"
#include "qgd_setup.hpp"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
using namespace qgd;

static const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
static const int32_t pt[6] = {0, 0, 0, 0, 0, 0};

static HostMesh readPrimitives(const std::string& path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot read " + path);
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
    if (!in) throw std::runtime_error("short file " + path);
    for (int i = 0; i < nPatches; ++i) {
        Patch p;
        p.name = "patch" + std::to_string(i);
        p.type = type[i]; p.start = start[i]; p.size = size[i];
        m.patches.push_back(p);
    }
    return m;
}

static HostMesh meshOf(const std::string& spec) {
    int nx, ny, nz, z0, z1;
    if (spec == "jitter11") {
        HostMesh m = makeBox(11, 9, 7, 0, 7, lo, hi, pt);
        jitterPoints(m, 0.15, 7); splitQuads(m, 3); splitEdges(m, 5);
        return m;
    }
    if (spec == "jitter24") {
        HostMesh m = makeBox(24, 16, 16, 0, 16, lo, hi, pt);
        jitterPoints(m, 0.15, 7);
        return m;
    }
    if (spec == "graded") {   // the last cell twice as long as the first, geometric
        const int n = 20;
        HostMesh m = makeBox(n, 8, 8, 0, 8, lo, hi, pt);
        const double r = std::pow(2.0, 1.0 / (n - 1));
        for (int32_t p = 0; p < m.nPoints; ++p) m.points[3 * (size_t)p] = (std::pow(r, m.points[3 * (size_t)p] * n) - 1.0) / (std::pow(r, (double)n) - 1.0);
        return m;
    }
    if (std::sscanf(spec.c_str(), "%dx%dx%d:%d-%d", &nx, &ny, &nz, &z0, &z1) == 5) return makeBox(nx, ny, nz, z0, z1, lo, hi, pt);
    if (std::sscanf(spec.c_str(), "%dx%dx%d", &nx, &ny, &nz) == 3) return makeBox(nx, ny, nz, 0, nz, lo, hi, pt);
    const size_t colon = spec.rfind(':');
    const int shardOf = colon == std::string::npos ? 0 : std::atoi(spec.c_str() + colon + 1);
    HostMesh m = readPrimitives(spec.substr(0, colon));
    if (shardOf > 0) {
        m.computeGeometry();
        const std::vector<int32_t> order = mortonOrder(m);
        renumberCells(m, order.data(), nullptr);
        std::vector<int32_t> cellStart;
        for (int r = 0; r <= shardOf; ++r) cellStart.push_back((int32_t)((int64_t)m.nCells * r / shardOf));
        m = extractShard(m, shardOf, cellStart.data(), shardOf / 2);
    }
    return m;
}

template <class Vec>
static void digest(const char* name, const Vec& v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(v[0]); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    std::printf("  %-10s %10zu  %016llx\n", name, v.size(), (unsigned long long)h);
}

static void digestMesh(const std::string& spec) {
    HostMesh m = meshOf(spec);
    m.computeGeometry();
    m.computeDerived();
    const StaticData s = buildStaticData(m);
    const FusedBlocks B = buildFusedBlocks(s);
    std::printf("%s\n", spec.c_str());
    std::printf("  blocks %d layer %d templates %d templated %d mismatches %d brick %d %d %d\n", B.nBlocks, B.nLayerBlocks, B.nTemplates, B.templated,
                B.templateMismatches, B.brick[0], B.brick[1], B.brick[2]);
    std::printf("  cap C %d V %d F %d E %d PE %d  max C %d V %d F %d Tot %d All %d Lds %d LdsImpl %d\n", B.capC, B.capV, B.capF, B.capE, B.capPE, B.maxC, B.maxV,
                B.maxF, B.maxTot, B.maxAll, B.maxLds, B.maxLdsImpl);
    std::printf("  packedW %d maxWeightOffset %d wRef %016llx  packedF %d classes %d maxFaceOffset %d fwRef %016llx fhRef %016llx %016llx %016llx %016llx\n", B.packedW,
                B.maxWeightOffset, (unsigned long long)B.wRef, B.packedF, B.nHfClasses, B.maxFaceOffset, (unsigned long long)B.fwRef, (unsigned long long)B.fhRef[0],
                (unsigned long long)B.fhRef[1], (unsigned long long)B.fhRef[2], (unsigned long long)B.fhRef[3]);
    std::printf("  faces %lld cells %lld cellsFull %lld verts %lld\n", (long long)B.facesComputed, (long long)B.cellsStaged, (long long)B.cellsStagedFull,
                (long long)B.vertsStaged);
    digest("hdr", B.hdr); digest("hdr2", B.hdr2); digest("cells", B.cells); digest("verts", B.verts); digest("faceLabel", B.faceLabel);
    digest("facePos", B.facePos); digest("vCount", B.vCount); digest("vPos", B.vPos); digest("vW", B.vW); digest("vW16", B.vW16);
    digest("fW16", B.fW16); digest("fKC", B.fKC); digest("nEntry", B.nEntry); digest("entry", B.entry);
    std::printf("  packedG %d maxGeoDict %d maxGeoOffset %d gvRef %016llx ghRef %016llx\n", B.packedG, B.maxGeoDict, B.maxGeoOffset, (unsigned long long)B.gvRef,
                (unsigned long long)B.ghRef);
    digest("gCode", B.gCode); digest("gOwn", B.gOwn); digest("gDict", B.gDict);
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "digest") == 0) {
        for (int a = 2; a < argc; ++a) digestMesh(argv[a]);
        return 0;
    }
    const int n = argc > 1 ? std::atoi(argv[1]) : 128;
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* w) { auto t = std::chrono::steady_clock::now(); std::printf("%-40s %8.2f s\n", w, std::chrono::duration<double>(t - t0).count()); t0 = t; };
    HostMesh m = makeBox(n, n, n, 0, n, lo, hi, pt); lap("makeBox");
    StaticData s = buildStaticData(m); lap("buildStaticData");
    FaceTiles t = buildFaceTiles(s, 128); lap("buildFaceTiles");
    FusedBlocks b = buildFusedBlocks(s); lap("buildFusedBlocks");
    std::printf("%d blocks, block builder %.3f s\n", b.nBlocks, b.buildSeconds);
    return 0;
}
