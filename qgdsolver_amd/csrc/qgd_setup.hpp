// qgd_setup.hpp -- static, per-mesh stencil data in the flat layouts the HIP
// kernels stream (built once on the host, uploaded by qgd_device_create).
//
// Layout rules (DESIGN.md "Data layout in HBM"):
//  * every per-face array is indexed by the GLOBAL face label (internal faces
//    first, then boundary faces) so internal- and boundary-face kernels share it
//  * streamed per-face data is SoA (one array per scalar) for coalesced loads
//  * gathered per-cell / per-vertex data is AoS records (one record = one
//    contiguous 16-B aligned chunk)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "qgd_fused_caps.hpp"
#include "qgd_mesh.hpp"

namespace qgd {

enum FaceKind : uint8_t { FK_QUAD = 0, FK_TRI = 1, FK_OTHER = 2, FK_SKIP = 3 };

struct StaticData {
    int32_t nP = 0, nF = 0, nIF = 0, nC = 0, nBF = 0;
    int32_t nGeomD = 3, ie1 = 0, ie2 = 1, ie3 = 2;
    bool hasTri = false;

    // ---- faces --------------------------------------------------------------
    RawVec<int32_t> own;     // nF   (RawVec: the per-face / per-cell tables are filled by parallel loops, qgd_setup.cpp)
    RawVec<int32_t> nei;     // nIF
    RawVec<int32_t> verts;   // 4*nF (tri: [3] = -1)
    RawVec<uint8_t> fkind;   // nF
    RawVec<double> Sf[3];    // nF each
    RawVec<double> magSf;    // nF
    RawVec<double> w;        // nF linear weights
    RawVec<double> hf;       // nF hQGDf
    RawVec<double> dn;       // nF: nonOrthDeltaCoeffs (internal), deltaCoeffs (boundary)
    // GaussVolPoint 3-D: the 10 (quad) / 13 (triangle) Gauss coefficients of a face are NOT stored: the face kernel
    // rebuilds them from the vertex coordinates and the two cell centres, which are gathered (and cached) instead
    // of streaming 80 B per face.  Boundary faces use the mirror point C_O + 2 (C_f - C_O) as "neighbour centre".
    RawVec<double> X;        // 3*nP: vertex coordinates (packed 24-B records)
    RawVec<double> Cc;       // 3*nC: cell centres (packed 24-B records)
    std::vector<double> bN;       // 4*nBF: mirror points of the boundary faces
    std::vector<double> bmvON;    // nBF
    // GaussVolPoint 2-D
    std::vector<int32_t> ip13;    // 2*nF (ip1, ip3)
    std::vector<double> c2d;      // 6*nF: c1,c2,c3,c4,mv42,mv13 (SoA: [k*nF+f])
    // leastSquares (internal faces)
    // leastSquares stencil as sliced ELL over the internal faces (64-face slices, entry e of face f at
    // (lsqSlice[f/64] + e)*64 + f%64): neighbour cell and the three components of wf2*Gdf
    std::vector<int32_t> lsqSlice;  // nSlices+1
    std::vector<uint8_t> lsqCnt;    // nIF
    std::vector<int32_t> lsqCell;
    std::vector<double> lsqGx, lsqGy, lsqGz;
    std::vector<uint8_t> lsqDeg;  // nIF
    std::vector<uint8_t> lsqBndZero;  // nBF: 1 on constraint patches (gradient left zero)
    std::vector<uint8_t> bSymm;       // nBF: 1 on symmetryPlane / symmetry / wedge patches (empty: none) -- scalar patch fields there have snGrad = 0 by type

    // ---- points -------------------------------------------------------------
    // point -> cells in sliced-ELL form: a slice is 64 consecutive points (one wavefront); entry i of the 64
    // points of slice s sits at (pcSlice[s] + i)*64 + lane, so every gather-list load of a wave is one
    // contiguous 256/512-B run.  Rows keep OpenFOAM's pointCells order (ascending cell label); patch points
    // have count 0.
    std::vector<int32_t> pcSlice; // nSlices+1, in rows of 64 entries
    std::vector<uint8_t> pcCount; // nP
    RawVec<int32_t> pcCell;  // padded entries: -1
    RawVec<double> pcW;
    std::vector<int32_t> bpPoint; // patch points
    std::vector<int32_t> bpOff;   // bpPoint.size()+1
    std::vector<int32_t> bpFace;  // boundary-face index (global label - nIF)
    std::vector<double> bpW;
    // Point constraints of VECTOR / TENSOR vertex fields (L0 assumption: volPointInterpolation::interpolateBoundaryField ends with
    // pointConstraints::constrain): per patch point (row i of bpPoint) the operations cpOff[i] .. cpOff[i+1], applied in order to the
    // weighted mean of the patch-face values.  kind 0: x = (x + transform(T, x))/2 with T = I - 2 nn -- the evaluate() of a
    // symmetryPlane (n = the patch normal) or symmetry (n = the point normal) point patch, in patch order; kind 1: x = transform(T, x)
    // -- a wedge point patch (T = I - nn) and, last, the patch-patch ("corner") constraint of points on the rim of one or more
    // constraint patches (T = I - nn | the edge direction squared | 0 for one | two | three independent normals).  Scalars are
    // untouched (transform is the identity on them).  Empty when the mesh has no symmetryPlane / symmetry / wedge patch.
    std::vector<int32_t> cpOff;   // bpPoint.size()+1 (empty: no constraints)
    std::vector<uint8_t> cpKind;
    std::vector<double> cpT;      // 9 per operation, row-major

    // ---- cells --------------------------------------------------------------
    // cell -> faces flux gather list, sliced-ELL like pc*; rows in ascending face label (== the summation order of
    // fvc::surfaceIntegrate); item = f (cell is owner, +) or ~f (cell is neighbour, -); empty/halo faces left out
    std::vector<int32_t> cfSlice; // nSlices+1
    std::vector<uint8_t> cfCount; // nC
    RawVec<int32_t> cfItem;
    RawVec<int32_t> cfNbr;   // like cfItem: the cell across the face, -1 for boundary faces
    // Storage order of the net face fluxes (CaseView::flux).  Internal face f keeps its five fluxes at position
    // fpos[f] of each SoA plane: faces are bucketed by their rank among the faces their owner owns (bucket 0 = every
    // cell's first owned face, in cell order, then bucket 1, ...), so that consecutive cells find their own faces AND
    // the faces they are the neighbour of (on a hexahedral box: the i-1, j-1 and k-1 faces) at consecutive positions.
    // Boundary faces stay at their label.  cfPos = cfItem with the label replaced by the position (same row order, ~pos
    // when the cell is the neighbour): the cell kernel's gather list.
    std::vector<int32_t> fpos;    // nIF
    RawVec<int32_t> cfPos;   // like cfItem
    std::vector<double> V;        // nC
    std::vector<double> hQGD;     // nC
    std::vector<uint8_t> ghost;   // nC cell role (empty when unsharded): 0 owned, 1 ghost, 2 owned + sent to a neighbour

    // ---- boundary faces -----------------------------------------------------
    std::vector<int32_t> bPatch;  // nBF patch index
    std::vector<double> hQGDb;    // nBF: hQGD boundary (= hQGDf boundary)

    // ---- halo -----------------------------------------------------------------
    std::vector<std::vector<int32_t>> haloGhost, haloSend, haloGhostBF, haloSendBF;  // one entry per halo slot

    int64_t bytes() const;
};

// build every table above; `needLsq` / `needGvp2` are derived from nGeometricD
StaticData buildStaticData(const HostMesh& m);

// ---- face tiles of the LDS-staged 3-D GaussVolPoint kernel ------------------------------------------------------------
// A tile is `fb` consecutive internal faces (one workgroup).  Its faces reference far fewer distinct cell and vertex
// records than 2 + 4 per face (blockMesh numbering, fb = 128: 130 cells and 175 vertices instead of 256 + 512), so the
// workgroup brings each distinct record in ONCE, as contiguous 16-B pieces, stages it in LDS and lets every face pick
// its six records from there: cells[]/verts[] list the distinct labels of each tile in ascending order (off[] = the
// two CSR offsets per tile), locC/locV hold each face's positions in those lists (16 bit each).
struct FaceTiles {
    int32_t fb = 0;                  // 0: not built (not a 3-D mesh or switched off)
    int32_t maxCells = 0, maxVerts = 0;   // over the staged tiles
    std::vector<int32_t> off;        // 2*(nTiles+1): {cell offset, vertex offset}
    std::vector<int32_t> spill;      // tiles with more distinct records than the caps below (e.g. the last rows of a box, whose
                                     // cells own one internal face each): empty lists here, they go through the gather kernel
    std::vector<int32_t> cells, verts;
    std::vector<uint32_t> locC;      // nIF: owner position | neighbour position << 16
    std::vector<uint32_t> locV;      // 2*nIF: v0 | v1 << 16,  v2 | v3 << 16 (absent vertex: 0)
};
// distinct records a tile may hold: what the kernel's fixed number of piece loads per thread covers
// (4, 3 and 5 rounds of 16-B pieces for cell RecA / RecB / vertex RecA).  A box in blockMesh numbering has fb + 3 cells and
// 11/8 fb vertices in all but the row-end tiles (< 1 %), which the tighter vertex cap leaves to the gather kernel: LDS per
// workgroup stays at 26.8 KB for fb = 128, six workgroups per CU.
inline int32_t faceTileCapCells(int32_t fb) { return fb + fb / 16; }
inline int32_t faceTileCapVerts(int32_t fb) { return ((fb * 23) / 16 + 7) / 8 * 8; }
FaceTiles buildFaceTiles(const StaticData& s, int32_t fb);


// ---- cell blocks of the fused face + cell kernel (QGD_FUSED; qgd_kernels.hip fusedFaceCellKernel) ---------------------------------
// A block is up to 128 cells that sit together in space (consecutive cells of a Morton order of the cell centres: an 8x4x4 brick on
// a uniform box) and EVERY internal face of those cells -- the faces on the block's surface are computed by the block on either side.
// One workgroup stages the distinct cell records (the block's own cells first, then the cells across its surface) and vertex records
// of those faces in LDS, computes the five net fluxes of each face into LDS, and advances its own cells out of LDS: the fluxes of
// internal faces never reach HBM.  Fixed strides (capC, capV, capF, capE), lists padded with their last entry.
struct FusedBlocks {
    int32_t nBlocks = 0;
    int32_t nLayerBlocks = 0;                         // a shard: the first nLayerBlocks blocks hold the cells a neighbour waits for
    int32_t capC = 0, capV = 0, capF = 0, capE = 0;   // strides: staged cells, staged vertices, faces, face entries per own cell
    int32_t maxC = 0, maxV = 0, maxF = 0;             // what the largest block uses (sizes the LDS)
    RawVec<int32_t> hdr;      // 4 per block: own cells, staged cells, staged vertices, faces
    RawVec<int32_t> cells;    // capC per block
    RawVec<int32_t> verts;    // capV per block
    RawVec<int32_t> faceLabel;   // capF per block: the global face label
    // The block's LOCAL TOPOLOGY -- per face the positions of its two cells and four vertices in the staged lists, per own cell its face
    // entries, per vertex the positions of its cells -- is stored per TEMPLATE, and hdr2[1] names a block's template: the interior bricks of
    // a structured region are all alike (a 400^3 box: 500 000 blocks, a few hundred templates), so 12.4 of the 31.3 KB a block streamed per step
    // in round 5 stay in L2 instead.  Blocks with a patch face (its entry is the face's own label) and the blocks of a jittered, renumbered mesh
    // (no two bricks list their cells alike) have templates of their own: the same bytes as before, read through the template id.
    int32_t nTemplates = 0, templated = 0;
    int32_t templateMismatches = 0;   // blocks whose fingerprint matched a template that their tables did not: each got a template of its own (a collision; 0 in practice)
    RawVec<uint32_t> facePos;    // 3 per face, capF faces per template: lo | ln << 16, v0 | v1 << 16, v2 | v3 << 16 (positions in the staged lists)
    // the vertex values formed inside the block (volPointInterpolation's inverse-distance weights, pointCells order): the cells around the
    // block's vertices that are neither its own nor across one of its faces ("extra": edge and corner neighbours) are staged too, behind
    // the others in `cells`; hdr2[0] = all staged cells.  Per vertex: its cells' positions in `cells` and the weights, entry-major
    // (capPE x capV per block); count 0 = a patch point, whose value the patch-point kernel has put into the vertex records.
    int32_t capPE = 0, maxTot = 0, maxAll = 0;        // cells per vertex; staged cells incl. extras / without them, of the largest block
    int32_t maxLds = 0;                               // LDS bytes of the records of the block that needs most (the kernel lays each block out by its own counts)
    int32_t maxLdsImpl = 0;                           // ... in the layout of the implicitDiffusion branch's assembly (fvc::grad(U) staged too, eight flux planes)
    RawVec<int32_t> hdr2;     // 4 per block: all staged cells, template, 0, 0
    RawVec<uint8_t> vCount;   // capV per block
    RawVec<uint16_t> vPos;    // capPE x capV per template
    RawVec<double> vW;        // capPE x capV per block
    // PACKED WEIGHTS (packFusedWeights below; QGD_FUSED_PACKED_W=0: never).  On a uniform hexahedral region every weight is 1/8 give or take
    // rounding, so the bit patterns of ALL weights of the mesh lie within a few thousand of each other: where capPE == 8 and their spread
    // is <= 65 535, a weight is kept as the signed 16-bit offset of its pattern from wRef (the midpoint pattern) -- 16 B per vertex
    // instead of 64, and bits(w) = wRef + offset gives the double back exactly.  Vertex-major: a vertex's eight offsets are one aligned
    // 16-B piece.  Entries beyond a vertex's count are 0.  What excludes a mesh is the spread alone: graded and unstructured meshes and a
    // jitter of the points beyond roughly 3e-12 of the cell size exceed it and keep vW alone; a smaller jitter moves the patterns by
    // thousands and still packs, with offsets that use all 16 bits (tests/packed_wide_recipes.py).
    int32_t packedW = 0;      // 1: vW16 / wRef hold every weight of vW
    int32_t maxWeightOffset = 0;   // the largest |offset| in vW16 (0 .. 32768; reporting only)
    int64_t wRef = 0;
    RawVec<int16_t> vW16;     // 8 x capV per block: vW16[(blk * capV + lv) * 8 + e]
    // PACKED FACE STREAMS (packFusedFaceStreams below; QGD_FUSED_PACKED_F=0: never; only where packedW == 1).  The linear weight w, hQGDf and
    // the kind of a block's face slots are static, so they can lie block-major in the kernel's face-slot order (slot i of block b at
    // b * capF + i, the order of faceLabel) and be read in the list round, without the label.  On a uniform mesh w is 1/2 give or take
    // rounding and hQGDf has one value per axis spacing: where, over every computed face slot, the patterns of w lie within 65 535 of each
    // other and those of hf fall into at most four classes that each do, a slot is one 32-bit word -- low half int16(bits(w) - fwRef), high
    // half int16(bits(hf) - fhRef[class]) -- and one byte, kind | class << 2: 5 B per face instead of 17 B gathered by label.  Padding
    // slots are zero.  The classes are cut greedily from the sorted patterns (class c starts at the smallest pattern beyond class c - 1's
    // 65 536), so they do not depend on the thread count; the references are the midpoint patterns, rounded up.
    int32_t packedF = 0;      // 1: fW16 / fKC / fwRef / fhRef hold w, hf and fkind of every computed face slot
    int32_t nHfClasses = 0;
    int32_t maxFaceOffset = 0;     // the largest |offset| in fW16, over both halves of every word (0 .. 32768; reporting only)
    int64_t fwRef = 0, fhRef[4] = {0, 0, 0, 0};
    RawVec<uint32_t> fW16;    // capF per block
    RawVec<uint8_t> fKC;      // capF per block
    // PACKED GEOMETRY (packFusedGeometry below; QGD_FUSED_PACKED_G=0: never; only where packedF == 1).  The centres of a block's own +
    // across-a-face cells, the coordinates of its vertices and V / hQGD of its own cells are static too, and on a mesh whose blocks see few
    // distinct coordinates per axis they carry little information.  Per block and per axis a dictionary of at most 16 reference patterns --
    // one set for the centres, one for the vertices, cut greedily from the block's sorted patterns (entry e starts at the smallest pattern
    // beyond the 4 096 of entry e - 1) -- and per coordinate one 16-bit code, entry << 12 | pattern - dictionary[entry]: bits = entry +
    // offset gives the double back exactly.  The codes lie in the kernel's own LDS slot order (slot q = 3 * list position + axis): thread t
    // of the 256 stages the centre slots t + 256 k (k < 4) and the vertex slots t + 256 k (k < 3), and its eight half words -- four centre
    // codes, three vertex codes, one spare -- are one aligned 16-B piece.  V and hQGD of own cell j are the two signed 16-bit offsets of one
    // word (low half from gvRef, high half from ghRef, the midpoint patterns of the mesh).  Slots beyond a block's counts are zero.
    int32_t packedG = 0;      // 1: gCode / gOwn / gDict / gvRef / ghRef hold Cc, X, V and hQGD of everything the blocks stage
    int32_t maxGeoDict = 0;   // the largest dictionary met, over blocks, sets and axes (1 .. 16; reporting only)
    int32_t maxGeoOffset = 0; // the largest 12-bit offset in gCode (0 .. 4095; reporting only)
    int64_t gvRef = 0, ghRef = 0;
    RawVec<uint16_t> gCode;   // 8 x 256 per block: gCode[(blk * 256 + t) * 8 + k] centre slot t + 256 k, [.. + 4 + k] vertex slot t + 256 k
    RawVec<uint32_t> gOwn;    // 128 per block
    RawVec<int64_t> gDict;    // 96 per block: [set * 48 + axis * 16 + entry], set 0 = centres, 1 = vertices; unused entries 0
    RawVec<uint8_t> nEntry;   // 128 per block: face entries of each own cell
    RawVec<int32_t> entry;    // capE x 128 per template, entry-major: (local face << 1) | (1: the cell is the neighbour, minus), or ~label of a boundary face
    int32_t brick[3] = {0, 0, 0};  // the lattice brick the blocks were cut from (8 x 4 x 4 unless another shape fills the blocks better; 0: count-based runs)
    double buildSeconds = 0.0;     // host time of buildFusedBlocks
    int64_t facesComputed = 0;     // over all blocks (a face between two blocks is computed by both)
    int64_t cellsStaged = 0, cellsStagedFull = 0, vertsStaged = 0;   // over all blocks: cell records staged (RecA), of which with RecB + centre; vertices formed
};
// LDS bytes of one block's records, from its counts of staged cells, own + across-a-face cells, vertices and faces (fusedFaceCellKernel lays
// each block out by its own counts at run time): RecA of every staged cell, RecB of the own + across-a-face ones, then vertex records +
// coordinates + centres, which the fluxes overwrite
constexpr int32_t fusedBlockLds(int32_t nTot, int32_t nAll, int32_t nV, int32_t nF) {
    return 48 * nTot + 32 * nAll + std::max(72 * nV + 24 * nAll, 40 * nF);
}
// ... in the layout of the implicitDiffusion branch's assembly, which reuses the vertex region for four flux planes, then the gradients of the
// own + across-a-face cells, then four planes again (qgd_kernels.hip fusedFaceCellKernel<..., IMPL>)
constexpr int32_t fusedBlockLdsImpl(int32_t nTot, int32_t nAll, int32_t nV, int32_t nF) {
    return 48 * nTot + 32 * nAll + std::max({72 * nV + 24 * nAll, 32 * nF, 72 * nAll});
}
// LDS a block's records may take so that three blocks (+ 3 KB of parked face entries each) share a CU's 160 KB: what an 8x4x4 brick needs
// (360 staged cells, 288 of them own or across a face, 225 vertices, 464 faces)
constexpr int32_t kFusedLdsTarget = fusedBlockLds(360, 288, 225, 464);
static_assert(kFusedLdsTarget == 48 * 360 + 32 * 288 + 72 * 225 + 24 * 288, "the LDS budget of three blocks per CU");
// keepFullWeights = false: vW is dropped once vW16 holds it (the device path: 8 x 8 B per vertex formed that nothing reads again)
FusedBlocks buildFusedBlocks(const StaticData& s, bool keepFullWeights = true);
// The packing rule on a block table whose nBlocks, capV, capPE, vCount and vW are filled: fills vW16 / wRef and sets packedW where the
// weights qualify (every entry decoded once and compared with vW bit for bit), leaves all three empty / 0 where they do not.  The
// result does not depend on the number of threads.  Returns packedW.
bool packFusedWeights(FusedBlocks& B);
// The same for the per-face streams, on a block table whose nBlocks, capF, hdr, faceLabel and packedW are filled: fills fW16 / fKC / fwRef /
// fhRef and sets packedF where s.w and s.hf of the computed face slots qualify (every slot decoded once and compared with s.w, s.hf and
// s.fkind of its face), leaves them empty / 0 where they do not or where packedW != 1.  Returns packedF.
bool packFusedFaceStreams(FusedBlocks& B, const StaticData& s);
// The same for the geometry, on a block table whose nBlocks, capC, capV, hdr, cells, verts and packedF are filled: fills gCode / gOwn / gDict /
// gvRef / ghRef and sets packedG where no block needs a 17th dictionary entry on an axis, every block's slots fit the kernel's piece loads
// and V and hQGD of the own cells each span at most 65 535 patterns (every entry decoded once and compared with s.Cc, s.X, s.V and s.hQGD),
// leaves them empty / 0 where not or where packedF != 1.  Returns packedG.
bool packFusedGeometry(FusedBlocks& B, const StaticData& s);
// a geometry code decoded as the kernel does it: dictionary entry + 12-bit offset, taken as a double
inline double fusedCoordFromCode(const int64_t* dictAxis, uint16_t code) {
    const int64_t bits = dictAxis[code >> 12] + (int64_t)(code & 4095);
    double x;
    std::memcpy(&x, &bits, 8);
    return x;
}
// Whether the device uses a block table, and the dynamic LDS of its launches: the records of the block that needs most (maxLds / maxLdsImpl),
// rounded to 16 B, then the parked face entries of the own cells, rounded to 256 B; ldsCell = where the parked entries start, in 8-B units.
// The tables are refused when they are empty; when the blocks come out small -- under 88 cells on average: every block costs a workgroup
// two face passes whatever it holds, and such a mesh is better off with the three kernels (5.0 against 4.4 ms per step on a 16 M-cell mesh
// with 67-cell blocks) -- unless the caller takes any blocks (anyBlocks: tests, probes); when a count exceeds what the kernels' 16-bit
// positions and budgets hold; and when the explicit layout needs more than ldsLimit, what one workgroup may ask for (blocks of <= 32
// cells are exempt from the builder's three-per-CU budget, so one fat polyhedral block could exceed it: such a mesh keeps the three
// kernels instead of failing in its first step).  ldsImpl is 0 where the implicitDiffusion layout alone exceeds the limit.
struct FusedLaunchPlan {
    bool use = false;
    int32_t lds = 0, ldsCell = 0, ldsImpl = 0, ldsCellImpl = 0;
};
FusedLaunchPlan planFusedLaunch(const FusedBlocks& B, int64_t nOwned, int64_t ldsLimit, bool anyBlocks);
inline double fusedWeightFromOffset(int64_t ref, int16_t off) {
    const int64_t bits = ref + (int64_t)off;
    double w;
    std::memcpy(&w, &bits, 8);
    return w;
}

}  // namespace qgd
