/*
 * qgd_amd.h -- C-ABI of the MI355X-native QGD face-flux path.
 *
 * This is the drop-in boundary for the per-timestep face-flux assembly of
 * QGDFoam (unicfdlab/QGDsolver).  Plain pointers and sizes only; no C++ or
 * torch types cross this boundary.  Every entry returns an int status
 * (QGD_OK == 0, negative == error) and never throws.
 *
 * Citations are to the Doxygen listings of the reference:
 *   /root/reference/docs/html/<name>_source.html, listing lines L..
 * (physical HTML line = listing line + 101).
 *
 * Reference interface each group replaces:
 *   qgd_fvsc_*            fvsc::grad / fvsc::div free functions
 *                         [fvsc_8H_source.html L46-68, fvsc_8C_source.html L87-167]
 *                         and the four fvscStencil virtuals Grad/Grad/Div/Div
 *                         [fvscStencil_8H_source.html L105-130]
 *   qgd_stencil_lookup    fvscStencil::New / lookupOrNew run-time selection by word
 *                         [fvscStencil_8C_source.html L59-118], with the scheme
 *                         checks of fvscOpName [fvsc_8C_source.html L47-85]
 *   qgd_case_update_fluxes  QGDFoam/updateFields.H + QGDFoam/updateFluxes.H
 *                         [QGDFoam_2updateFields_8H_source.html L45-80,
 *                          QGDFoam_2updateFluxes_8H_source.html L41-139]
 *   qgd_case_step         one pass of the QGDFoam while-loop body
 *                         [QGDFoam_8C_source.html L90-163]
 *   qgd_case_get_field    QGDThermo accessors tauQGDf/hQGDf/tauQGD/hQGD/muQGD/
 *                         alphauQGD/c/p/rho/mu [QGDThermo_8H_source.html L99-135]
 *                         and the registered face fields the qgdFlux BC reads by
 *                         name ("phiwStar", "tauQGDf")
 *                         [qgdFluxFvPatchScalarField_8C_source.html L166-192]
 *
 * Layout conventions (same as OpenFOAM's):
 *   - labels are int32, scalars are fp64
 *   - vectors are 3 contiguous doubles, tensors 9 row-major doubles,
 *     T[3*i+j]; a face gradient of a vector is out[3*i+j] = d_i U_j
 *     [leastSquaresStencil_8C_source.html L155-165]
 *   - a surface field is nFaces records: internal faces 0..nInternalFaces-1
 *     followed by the boundary faces patch by patch in mesh order.  Faces of
 *     `empty` patches keep a (zero) slot so that a record is addressed by its
 *     global face label (OpenFOAM gives those patches size 0).
 *   - a boundary ("patch") field is nFaces-nInternalFaces records addressed by
 *     (global face label - nInternalFaces).
 */
#ifndef QGD_AMD_H
#define QGD_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
enum {
    QGD_OK = 0,
    QGD_ERR_INVALID = -1,     /* bad argument / inconsistent sizes               */
    QGD_ERR_NO_DEVICE = -2,   /* no HIP device: the product path has NO CPU fallback */
    QGD_ERR_HIP = -3,         /* a HIP runtime call failed (see qgd_last_error)  */
    QGD_ERR_SCHEME = -4,      /* scheme rejected, e.g. leastSquares on a 3-D mesh
                                 [fvsc_8C_source.html L60-63]                     */
    QGD_ERR_UNKNOWN_NAME = -5,/* unknown stencil / field / model word            */
    QGD_ERR_NOT_IMPLEMENTED = -6 /* mirrors notImplemented(...) of the base class
                                 [fvscStencil_8H_source.html L105-130]           */
};

/* ---- patch (mesh boundary) types: the fvPatch classes the path tests for -- */
enum {
    QGD_PATCH_GENERIC = 0,        /* patch / wall: ordinary                      */
    QGD_PATCH_EMPTY = 1,          /* emptyFvPatch (2-D / 1-D cases)              */
    QGD_PATCH_SYMMETRYPLANE = 2,  /* symmetryPlaneFvPatch                        */
    QGD_PATCH_SYMMETRY = 3,       /* symmetryFvPatch                             */
    QGD_PATCH_WEDGE = 4,          /* wedgeFvPatch                                */
    QGD_PATCH_CYCLIC = 5,         /* coupled, not processor                      */
    QGD_PATCH_HALO = 6            /* cut plane of a cell-range shard (plays the
                                     role of processorFvPatch): its faces are
                                     never integrated, ghost cells behind it are
                                     refreshed by the halo exchange              */
};

/* ---- boundary-condition kinds of the QGDFoam case ------------------------- */
enum {
    QGD_BC_ZEROGRADIENT = 0,
    QGD_BC_FIXEDVALUE = 1,
    QGD_BC_SLIP = 2,       /* basicSymmetry: U only (also used on symmetryPlane)  */
    QGD_BC_QGDFLUX = 3,    /* p only: qgdFluxFvPatchScalarField
                              [qgdFluxFvPatchScalarField_8C_source.html L159-197] */
    QGD_BC_NONE = 4,       /* empty / halo patches                                */
    QGD_BC_QHDFLUX = 5     /* p of the QHD case only: qhdFlux fed by the registered flux, gradient =
                              -(phiw/tauQGDf*rhof/|Sf|) [qhdFluxFvPatchScalarField_8C_source.html L193-203], as in the
                              QHD solvers that register "phiwStar" (mulesQHDFoam/createFields.H); QHDFoam itself does not,
                              there the patch keeps the gradient of its file = QGD_BC_QGDFLUX with that value */
};

/* ---- fvsc stencil words [fvsc_8C_source.html L60-65] ---------------------- */
enum {
    QGD_FVSC_REDUCED = 0,
    QGD_FVSC_LEASTSQUARES = 1,
    QGD_FVSC_GAUSSVOLPOINT = 2
};

/* ---- opaque handles -------------------------------------------------------- */
typedef struct qgd_mesh_s* qgd_mesh_t;     /* host polyMesh + derived geometry  */
typedef struct qgd_device_s* qgd_device_t; /* device-resident mesh + stencils   */
typedef struct qgd_case_s* qgd_case_t;     /* a QGDFoam case on one device      */

/* ---- library ---------------------------------------------------------------- */
/* Bumped whenever an options struct grows or an entry changes its meaning (3: round 3). */
#define QGD_ABI_VERSION 9
const char* qgd_version(void);
/* sizes[0..2] = sizeof(qgd_case_options), sizeof(qgd_qhd_options), sizeof(qgd_poisson_control) as THIS library was built,
 * sizes[3] = its QGD_ABI_VERSION: a host compiled against another header compares before it passes a struct (the structs
 * carry no size member; the library copies sizeof(its own) bytes). */
int qgd_struct_sizes(int64_t sizes[4]);
/* Last error text of the calling thread (never NULL). */
const char* qgd_last_error(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int qgd_device_count(void);

/* ---- mesh (host side, plain C++; no device needed) ------------------------ */

/* polyMesh arrays exactly as constant/polyMesh/{points,faces,owner,neighbour,
 * boundary}: faces in upper-triangular order, boundary faces grouped per patch.
 * Arrays are copied.  Geometry (Sf, Cf, C, V) is computed with OpenFOAM's
 * face/cell decomposition rules unless supplied via qgd_mesh_set_geometry. */
int qgd_mesh_create(int32_t nPoints, const double* points,
                    int32_t nFaces, const int32_t* faceOffsets /*nFaces+1*/,
                    const int32_t* facePoints,
                    int32_t nInternalFaces, const int32_t* owner /*nFaces*/,
                    const int32_t* neighbour /*nInternalFaces*/,
                    int32_t nCells,
                    int32_t nPatches, const int32_t* patchStart,
                    const int32_t* patchSize, const int32_t* patchType,
                    qgd_mesh_t* out);

/* Structured box in blockMesh numbering: cell i + nx*(j + ny*k), internal faces
 * sorted by (owner, neighbour), six patches xMin,xMax,yMin,yMax,zMin,zMax.
 * patchTypes[6] gives the QGD_PATCH_* of each.  kLo/kHi select a k-slab
 * [kLo,kHi) of a taller box of nzGlobal cells (kLo=0,kHi=nz for the whole box);
 * z-coordinates stay those of the global box so a shard is bit-identical to the
 * same cells of the global mesh. */
int qgd_mesh_box(int32_t nx, int32_t ny, int32_t nzGlobal,
                 int32_t kLo, int32_t kHi,
                 const double lo[3], const double hi[3],
                 const int32_t patchTypes[6],
                 qgd_mesh_t* out);

/* Forward-facing-step planform (one cell thick in z): nx*ny cells with the
 * block [ixStep,nx) x [0,iyStep) removed.  Patches: inlet, outlet, bottom,
 * top, step (walls of the obstacle), frontAndBack (empty). */
int qgd_mesh_forward_step(int32_t nx, int32_t ny, int32_t ixStep, int32_t iyStep,
                          double lx, double ly, double lz, qgd_mesh_t* out);

/* Move every point by jitter*h*uniform(-1,1) per coordinate (boundary points
 * slide in their plane only), then recompute geometry.  Test helper for
 * non-orthogonal hexahedra. */
int qgd_mesh_jitter(qgd_mesh_t m, double amplitude, uint64_t seed);
/* Split every `stride`-th internal and boundary quad into two triangles
 * (cells stay closed polyhedra): exercises the triangle branch
 * [GaussVolPointBase3D_8C_source.html L161-318]. */
int qgd_mesh_split_quads(qgd_mesh_t m, int32_t stride);
/* Insert a mid-edge vertex on edge 0 of every `stride`-th internal quad; every face sharing that edge gains the vertex
 * (pentagons, hexagons): exercises the "other faces" fallback to nf*snGrad
 * [GaussVolPointBase3D_8C_source.html L759-768].  Test helper. */
int qgd_mesh_split_edges(qgd_mesh_t m, int32_t stride);

/* ---- renumbering and cell-range sharding of any polyMesh ("ranges after a bandwidth-reducing
 * renumbering"; stands in for OpenFOAM's renumberMesh / decomposePar, which are not part of the reference tree) ---- */
/* Relabel the cells in place, newOfOld[old cell] = new cell (a permutation).  Internal faces are re-oriented and
 * re-sorted into upper-triangular order, boundary faces keep their labels, points are relabelled to follow their
 * cells (by the lowest new cell label using them).  faceNewOfOld (nFaces, may be NULL)
 * receives each old face's new label, or -1-label when the face was reversed (fluxes change sign). */
int qgd_mesh_renumber(qgd_mesh_t m, const int32_t* newOfOld, int32_t* faceNewOfOld);
/* newOfOld (nCells) of a reverse Cuthill-McKee ordering of the face-neighbour graph. */
int qgd_mesh_rcm_order(qgd_mesh_t m, int32_t* newOfOld);
/* newOfOld (nCells) of the Morton (Z-curve) order of the cell centres: spatial neighbours stay close in memory at
 * every scale (cache locality on the device); also a reasonable order to cut cell ranges from. */
int qgd_mesh_morton_order(qgd_mesh_t m, int32_t* newOfOld);
/* The shard of `rank` when the cells of `global` are cut into the contiguous ranges cellStart[r]..cellStart[r+1]
 * (cellStart[0]=0, cellStart[nRanks]=nCells): owned cells + one vertex-connected ghost layer (what
 * volPointInterpolation and the leastSquares stencil reach, extendedFaceStencilFindNeighbours_8C_source.html L55-80),
 * all faces of those cells, the global patches (same indices, possibly empty) followed by one QGD_PATCH_HALO patch,
 * and one halo slot per neighbouring rank.  qgd_mesh_get names of a shard: "cellGlobal","faceGlobal" (-1-label when
 * reversed),"pointGlobal","haloPeer","haloGhost<slot>","haloSend<slot>". */
int qgd_mesh_shard(qgd_mesh_t global, int32_t nRanks, const int32_t* cellStart, int32_t rank, qgd_mesh_t* out);
/* Translational cyclic patch pairs served by ghost cells.  The reference's stencils reach across a coupled patch through
 * patchNeighbourField and the true neighbour centre [GaussVolPointBase3D_8C_source.html L398-415, L588, L688, L783-794;
 * extendedFaceStencilScalarGrad_8C_source.html L90-101]; here the two halves of each pair are glued: `out` is the mesh followed by one
 * vertex-connected layer of translated copies of its own cells behind every half (diagonal copies at the edges / corners where several pairs
 * meet), the pairs' faces turned into internal faces between a real cell and a copy, the cyclic patches left empty (same indices), a
 * trailing QGD_PATCH_HALO patch, and halo slots whose messages stay on the rank: qgd_mesh_get "haloSelf" names, per slot, the slot whose
 * packed message it unpacks.  pairs = 2 * nPairs patch indices {A, B} with face i of A = face i of B shifted by one vector (checked:
 * rotational pairs are refused with QGD_ERR_NOT_IMPLEMENTED); nPairs = 0 pairs consecutive cyclic patches.  Real cells, points and patch
 * faces keep their labels ("cellGlobal" = the original of every cell).  A case on such a mesh steps with plain qgd_case_step (explicit branch):
 * the library refreshes the copies from their originals after every step, on the case's stream.  The copies belong to the library: what
 * qgd_case_set_fields is handed for them is never computed on -- qgd_case_step and qgd_case_update_fluxes give them their originals' records
 * first.  qgd_case_step_phase is refused on such a device (QGD_ERR_INVALID, "periodic device"): between two phases nothing would refresh
 * the copies.  qgd_case_set_bc asks for a new qgd_case_set_fields, as on every mesh, and the copies are refreshed again after it. */
int qgd_mesh_unroll_cyclic(qgd_mesh_t mesh, int32_t nPairs, const int32_t* pairs, qgd_mesh_t* out);
/* number of halo slots (neighbouring shards) of a mesh; 0 when unsharded, 2 for a qgd_mesh_box slab */
int qgd_mesh_halo_slots(qgd_mesh_t m, int32_t* nSlots);

/* The faceSet "degenerateStencilFaces" of the leastSquares stencil [leastSquaresStencil_8C_source.html L58-133]: faces the user
 * wants treated like the ones whose weight matrix is degenerate, i.e. the face gradient falls back to nf * snGrad
 * [extendedFaceStencilScalarGrad_8C_source.html L76-83].  Internal face labels count (the listing keeps boundary ones only on
 * processor patches); the list follows the faces through qgd_mesh_renumber / qgd_mesh_shard.  Call before qgd_device_create.
 * qgd_mesh_get name: "degenerateFaces". */
int qgd_mesh_set_degenerate_faces(qgd_mesh_t m, int32_t n, const int32_t* faces);
int qgd_mesh_set_geometry(qgd_mesh_t m, const double* Sf, const double* Cf,
                          const double* C, const double* V);
int qgd_mesh_free(qgd_mesh_t m);

/* sizes[0..6] = nPoints, nFaces, nInternalFaces, nCells, nPatches,
 *               nFacePoints (sum of face sizes), nGeometricD */
int qgd_mesh_sizes(qgd_mesh_t m, int64_t sizes[7]);
/* Copy out a named array: "points","faceOffsets","facePoints","owner",
 * "neighbour","patchStart","patchSize","patchType" (int32 / double as natural),
 * "Sf","magSf","Cf","C","V","weights","deltaCoeffs","nonOrthDeltaCoeffs".
 * outBytes < 0 asks for the size: *(int64_t*)out receives the array's length in bytes. */
int qgd_mesh_get(qgd_mesh_t m, const char* name, void* out, int64_t outBytes);

/* ---- device mesh + fvsc operators ----------------------------------------- */

/* Upload the mesh to HIP device `deviceId` and build the static stencil data.
 * Fails with QGD_ERR_NO_DEVICE when no GPU is present. */
int qgd_device_create(qgd_mesh_t m, int deviceId, qgd_device_t* out);
/* The same with the caller's choice about the block tables of QGDFoam's fused explicit step (qgd_case_fused_info; 3-D meshes only: ~30 KB per
 * block of 128 cells on the device and seconds of host set-up at tens of millions of cells), instead of the QGD_FUSED environment variable:
 *   QGD_DEVICE_NO_FUSED_TABLES   do not build them: a device whose cases never run the fused step (QHDFoam, implicitDiffusion, adjustTimeStep
 *                                with QGD_FUSED_ADJUST=0, reduced / leastSquares stencils) -- every case then steps with the separate kernels;
 *   QGD_DEVICE_FUSED_ANY_BLOCKS  build them and use them whatever the blocks look like (the default leaves a mesh whose blocks average under
 *                                88 cells to the separate kernels, which are faster there).
 * flags = 0 is qgd_device_create. */
#define QGD_DEVICE_NO_FUSED_TABLES 1
#define QGD_DEVICE_FUSED_ANY_BLOCKS 2
int qgd_device_create_with(qgd_mesh_t m, int deviceId, int32_t flags, qgd_device_t* out);
/* Ownership (fvscStencil_8C_source.html L57, L104-117: the reference's stencils live in the mesh's registry and die with it):
 * every case (qgd_case_t, qgd_qhd_case_t) keeps a pointer to the device it was created on and uses its stream until it is
 * freed, so free the cases BEFORE their device: qgd_device_free returns QGD_ERR_INVALID (and frees nothing) while cases created on
 * the device are still open.  The Python mirror enforces the order (fvsc.Device.close frees the cases still open on it first). */
int qgd_device_free(qgd_device_t d);

/* Run-time selection by word, like fvscStencil::New: "reduced",
 * "leastSquares", "leastSquaresOpt" (alias of leastSquares' serial formula),
 * "GaussVolPoint".  Applies the checks of fvscOpName: leastSquares* is refused
 * on 3-D meshes (QGD_ERR_SCHEME); unknown word -> QGD_ERR_UNKNOWN_NAME. */
int qgd_stencil_lookup(qgd_device_t d, const char* word, int* stencilId);

/* The four fvscStencil operators.  cell = nCells*ncomp, bnd = boundary (patch)
 * values nBoundaryFaces*ncomp, out = nFaces*ncompOut, all HOST pointers (the
 * OpenFOAM adapter hands over Field<Type>::cdata()).
 *   grad_s : ncomp 1 -> 3      grad_v : ncomp 3 -> 9
 *   div_v  : ncomp 3 -> 1      div_t  : ncomp 9 -> 3
 * The patch surface-normal gradient the boundary-face rules need is
 * deltaCoeffs*(bnd - internal), fvPatchField::snGrad (L0). */
int qgd_fvsc_grad_s(qgd_device_t d, int stencilId, const double* cell,
                    const double* bnd, double* out);
int qgd_fvsc_grad_v(qgd_device_t d, int stencilId, const double* cell,
                    const double* bnd, double* out);
int qgd_fvsc_div_v(qgd_device_t d, int stencilId, const double* cell,
                   const double* bnd, double* out);
int qgd_fvsc_div_t(qgd_device_t d, int stencilId, const double* cell,
                   const double* bnd, double* out);

/* The same four operators, qgdInterpolate, the QHD flux block and the species block on DEVICE pointers (buffers of
 * qgd_device_alloc or any allocation of this HIP device): same layouts, nothing staged, nothing crosses PCIe, stream-ordered on
 * the device handle's own stream -- qgd_device_sync waits.  For hosts whose fields already live in HBM (level 1 of
 * INTEGRATION.md without the 80 ms of PCIe per step the host-pointer entries cost at 8 M cells).  The struct members of
 * qgd_qhd_inputs / qgd_qhd_outputs are device pointers here.  qgd_device_copy: a plain synchronous copy for callers that hold
 * no HIP runtime of their own (toDevice != 0: host -> device). */
int qgd_fvsc_grad_s_dev(qgd_device_t d, int stencilId, const double* cellDev, const double* bndDev, double* outDev);
int qgd_fvsc_grad_v_dev(qgd_device_t d, int stencilId, const double* cellDev, const double* bndDev, double* outDev);
int qgd_fvsc_div_v_dev(qgd_device_t d, int stencilId, const double* cellDev, const double* bndDev, double* outDev);
int qgd_fvsc_div_t_dev(qgd_device_t d, int stencilId, const double* cellDev, const double* bndDev, double* outDev);
int qgd_interpolate_dev(qgd_device_t d, int32_t ncomp, const double* cellDev, const double* bndDev, double* outDev);
int qgd_device_sync(qgd_device_t d);
int qgd_device_copy(qgd_device_t d, void* dst, const void* src, int64_t bytes, int toDevice);
/* The leastSquares stencil of internal face `face` as the device holds it: the cells in the order they are summed, which is the order
 * the reference builds [extendedFaceStencilFindNeighbours_8C_source.html L48-84: the face's points in order, each point's cells in
 * pointCells() order, first occurrence kept].  *count = their number (the first `cap` are written).  Diagnostic entry (a few small
 * copies per call): tests/test_ref_expr_gpu.py compares it with the order executed from the listing text.  QGD_ERR_SCHEME on 3-D meshes. */
int qgd_device_lsq_stencil(qgd_device_t d, int32_t face, int32_t* cells, int32_t cap, int32_t* count);

/* Where the time of the last qgd_fvsc_* call on this device went: ms[0] = host -> device copies, ms[1] = kernels (HIP events),
 * ms[2] = device -> host copy.  Pageable caller memory moves through two pinned staging chunks in a double-buffered
 * pipeline; buffers of the persistent per-device workspace are reused from call to call (no allocation per call). */
int qgd_device_op_times(qgd_device_t d, double ms[3]);

/* How the internal faces of a 3-D mesh go through the GaussVolPoint flux kernel: info[0] = faces per tile (workgroup) of the
 * LDS-staged kernel, 0 when every face goes through the gather kernel (not a 3-D mesh, QGD_FTILE=0); info[1] = tiles;
 * info[2] = tiles left to the gather kernel (more distinct cell / vertex records than the staged kernel brings in);
 * info[3] = LDS bytes per workgroup.  Both kernels do the arithmetic of GaussVolPointBase3D_8C_source.html L346-389,
 * L488-513 + QGDFoam_2updateFluxes_8H_source.html L41-139 in the same order: results are bit-identical. */
int qgd_device_face_tiles(qgd_device_t d, int64_t info[4]);
/* The block tables of the fused explicit step on this device (all 0 when they were not built or not accepted; qgd_case_fused_info says whether
 * a case uses them): info[0] = blocks, [1] = of which the leading boundary-layer blocks of a shard, [2] = distinct templates of the blocks'
 * local topology (per-face list positions, per-cell face entries, per-vertex cell positions: blocks that are alike share one, so on a
 * structured mesh those tables stay in L2 instead of being streamed per block per step), [3] = LDS bytes per workgroup, [4] = bytes of a
 * block's own lists (labels, weights, counts), [5] = bytes of one template, [6] = host milliseconds the builder took, [7] = the lattice brick
 * the blocks were cut from, bx | by << 8 | bz << 16 (0: count-based runs of the Morton order); bit 24 of [7] = the vertex interpolation
 * weights are kept as 16-bit offsets from one reference bit pattern (a mesh whose weights all lie within 65 535 patterns of each other, e.g.
 * a uniform hexahedral region; QGD_FUSED_PACKED_W=0: never) -- [4] counts 2 bytes per weight then, not 8; bit 25 of [7] = the per-face streams w, hQGDf and kind of a
 * block's face slots lie block-major too, as two 16-bit offsets and one byte per slot (only with bit 24; QGD_FUSED_PACKED_F=0: never) --
 * [4] counts those 5 bytes per face slot then.  What the packed tables hold, for tests and reports (0 where they were not built): bits 26..28
 * of [7] = the classes of hQGDf (1..4), bits 29..44 = the largest |offset| among the vertex-weight offsets (0..32768), bits 45..60 = the
 * largest |offset| among the face words, over w and hQGDf (0..32768).  Bit 61 of [7] = the geometry the blocks stage -- cell centres, vertex
 * coordinates, V and hQGD of the own cells -- lies block-major too, as 16-bit dictionary codes and offsets (only with bit 25;
 * QGD_FUSED_PACKED_G=0: never); [4] counts those 5 376 bytes per block then.  [6] holds the milliseconds in its low 32 bits; above them, for
 * tests and reports: bits 32..36 = the largest dictionary of a block's axis (1..16), bits 40..51 = the largest 12-bit offset among the
 * codes (0..4095). */
int qgd_device_fused_blocks(qgd_device_t d, int64_t info[8]);

/* qgdInterpolate / linearInterpolate [QGDInterpolate_8H_source.html L38-67]: face = w*(phi_O - phi_N) + phi_N, patch faces
 * take the patch value.  cell nCells*ncomp, bnd nBoundaryFaces*ncomp, out nFaces*ncomp (HOST pointers), ncomp in 1..9. */
int qgd_interpolate(qgd_device_t d, int32_t ncomp, const double* cell, const double* bnd, double* out);
/* qgdFlux [QGDInterpolate_8H_source.html L76-118] without a divSchemes entry: out = flux*psif (flux nFaces, psif and out
 * nFaces*ncomp).  Pure host arithmetic (one multiply per value): kept so call sites read like the reference. */
int qgd_flux(qgd_device_t d, int32_t ncomp, const double* flux, const double* psif, double* out);
/* qgdFlux WITH a divSchemes entry `Gauss upwind` for the flux's name [QGDInterpolate_8H_source.html L86-104 -> fvc::flux]:
 * out = flux * (pos0(flux)*(psi_O - psi_N) + psi_N) on internal faces, flux * patch value on patch faces (`Gauss linear` is qgd_flux
 * on the linear psif: the same numbers).  flux nFaces, cell nCells*ncomp, bnd nBoundaryFaces*ncomp, out nFaces*ncomp, HOST pointers. */
int qgd_flux_upwind(qgd_device_t d, int32_t ncomp, const double* flux, const double* cell, const double* bnd, double* out);
/* Static QGD length scales of the mesh [QGDCoeffs_8C_source.html L298-376]: name = "hQGD" (nCells), "hQGDf" (nFaces),
 * "hQGD.boundary" (nBoundaryFaces).  The QHD tau closures (constTau, HbyUQHD, T0byGr, H2bynuQHD) are one line each on
 * top of these and qgd_interpolate; see qgdsolver_amd/qhdfoam.py. */
int qgd_device_get(qgd_device_t d, const char* name, double* out, int64_t outDoubles);

/* ---- QHDFoam flux assembly (stateless, host pointers) -------------------- */
/* The face-flux parts of the QHDFoam step: QHDFoam/updateFields.H L36-73 (gradients, interpolations, BdFrc),
 * QHDFoam/updateFluxes.H L33-38 (phiu, phiwo, taubyrhof), QHDUEqn.H L36-43 (gradPf, Wf, phiUf) and QHDTEqn.H
 * L65-66 (phiTf, phiTauTReg).  The implicit pressure Poisson solve between them (QHDpEqn.H L35-47) stays with the
 * caller: call once with p = phi = NULL for the first group, again with p and phi for the rest (or once with
 * everything).  cell arrays: nCells*ncomp, patch arrays: nBoundaryFaces*ncomp, face arrays: nFaces*ncomp. */
typedef struct qgd_qhd_inputs {
    const double* U;   const double* Ub;     /* 3 */
    const double* T;   const double* Tb;     /* 1 */
    const double* p;   const double* pb;     /* 1, nullable */
    const double* rho; const double* rhob;   /* 1 */
    const double* tauQGDf;                   /* nFaces: thermo.tauQGDf() of the chosen QGDCoeffs model */
    const double* phi;                       /* nFaces, nullable: phiu - phiwo + pEqn.flux() */
    double beta;                             /* thermal expansion coefficient */
    double g[3];                             /* gravitational acceleration */
} qgd_qhd_inputs;
typedef struct qgd_qhd_outputs {             /* every pointer may be NULL */
    double* gradUf;      /* 9: fvsc::grad(U) */
    double* gradTf;      /* 3: fvsc::grad(T) */
    double* phiu;        /* 1 */
    double* phiwo;       /* 1 */
    double* taubyrhof;   /* 1 */
    double* gradPf;      /* 3: needs p */
    double* Wf;          /* 3: needs p */
    double* phiUf;       /* 3: needs p and phi */
    double* phiTf;       /* 1: needs phi */
    double* phiTauTReg;  /* 1 */
} qgd_qhd_outputs;
int qgd_qhd_fluxes(qgd_device_t d, int stencilId, const qgd_qhd_inputs* in, qgd_qhd_outputs* out);
int qgd_qhd_fluxes_dev(qgd_device_t d, int stencilId, const qgd_qhd_inputs* in, qgd_qhd_outputs* out);   /* device pointers */

/* Species flux block -- reactingLagrangianQGDFoam_2updateFluxes_8H_source.html L117-132, one species:
 *     gradYf = fvsc::grad(Y);  phiJmY = qgdFlux(phiJm, Y, Yf);  dydtflux = -phi*tauQGDf*(Uf & gradYf);
 *     phiJmY += dydtflux;  diffusiveFlux = dydtflux;
 * Y[nCells], Yb[nBoundaryFaces], U[3 nCells], Ub[3 nBoundaryFaces] (patch values after their BCs), phiJm, phi, tauQGDf [nFaces]
 * as the QGDFoam block produced them (qgd_case_get_field "phiJm","phi","tauQGDf").  Out: phiJmY, diffusiveFlux [nFaces],
 * gradYf [3 nFaces] (may be NULL).  What QGDYEqn_8H_source.html L35-93 then does with them stays with the caller. */
int qgd_species_flux(qgd_device_t d, int stencilId, const double* Y, const double* Yb, const double* U, const double* Ub,
                     const double* phiJm, const double* phi, const double* tauQGDf, double* phiJmY, double* diffusiveFlux,
                     double* gradYf);
int qgd_species_flux_dev(qgd_device_t d, int stencilId, const double* Y, const double* Yb, const double* U, const double* Ub,
                         const double* phiJm, const double* phi, const double* tauQGDf, double* phiJmY, double* diffusiveFlux,
                         double* gradYf);
/* The species equation itself, one species, explicit branch -- QGDYEqn_8H_source.html L44-45, L67-86:
 *     solve(fvm::ddt(rho,Yi) + fvc::div(phiJmYi) - fvc::laplacian(muf/ScNumbers[i],Yi) == combustion->R(Yi) + parcels.SYi(i, Yi));
 *     diffusiveFlux[i] += (muf/ScNumbers[i]) * fvc::snGrad(Yi.oldTime()) * mesh.magSf();   Yi.max(0.0);
 * with the right-hand side handed in as ONE explicit source field Su [nCells] (kg/m^3/s; NULL: none) -- combustion and parcels stay with
 * the caller.  Y [nCells], Yb [nBoundaryFaces] (old time level, patch values after their BCs), rhoOld, rho [nCells] (before / after
 * QGDRhoEqn), phiJmY [nFaces] (qgd_species_flux), muf [nFaces] (qgd_case_get_field "muf"), Sc = ScNumbers[i], deltaT.
 * In/out: diffusiveFlux [nFaces].  Out: Ynew [nCells].  Euler ddt, fvc::div = surfaceIntegrate in ascending face label, Gauss laplacian
 * with the uncorrected snGrad (L0).  The inert species (L65 / L83, L90-91: Y_inert = 1 - sum, diffusiveFlux_inert -= diffusiveFlux_i)
 * is two axpys over these arrays and stays with the caller (qgdsolver_amd.qgdfoam.QGDYEqn does it). */
int qgd_species_step(qgd_device_t d, const double* Y, const double* Yb, const double* rhoOld, const double* rho, const double* phiJmY,
                     const double* muf, double Sc, double deltaT, const double* Su, double* diffusiveFlux, double* Ynew);
int qgd_species_step_dev(qgd_device_t d, const double* Y, const double* Yb, const double* rhoOld, const double* rho, const double* phiJmY,
                         const double* muf, double Sc, double deltaT, const double* Su, double* diffusiveFlux, double* Ynew);   /* device pointers */   /* device pointers */

/* The same equation, implicitDiffusion branch -- QGDYEqn_8H_source.html L47-66:
 *     fvScalarMatrix YEqn(fvm::ddt(rho,Yi) + fvc::div(phiJmYi) - fvm::laplacian(muf/ScNumbers[i],Yi) == combustion->R(Yi) + parcels.SYi(i, Yi));
 *     YEqn.solve();   diffusiveFlux[i] += YEqn.flux();   Yi.max(0.0);
 * Arguments as above plus fixedValueFace [nBoundaryFaces] (1: the face belongs to a fixedValue patch of Yi, value Yb: diagonal and source
 * coefficients |Sf| delta (muf/Sc); 0: zeroGradient, no contribution; NULL: all zeroGradient), and the controls fvSolution gives the
 * solver of Yi: tolerance on OpenFOAM's normalised residual, maxIter.  YEqn.flux() is the matrix's own face flux (L0 fvMatrix::flux) of
 * the NEW Yi: -a_f (Y_N - Y_O) inside, -a_b (Y_b - Y_P) on fixedValue faces -- the sign "- fvm::laplacian" gives it, opposite to the
 * explicit branch's +(muf/Sc) snGrad |Sf| of L82; replicated as listed.  info (host) = {iterations, initial, final residual}.  Solved by
 * the library's device-resident solver (Chebyshev iteration, or conjugate gradients with QGD_IMPL_SOLVER=pcg); one device, no shards. */
int qgd_species_step_implicit(qgd_device_t d, const double* Y, const double* Yb, const uint8_t* fixedValueFace, const double* rhoOld,
                              const double* rho, const double* phiJmY, const double* muf, double Sc, double deltaT, const double* Su,
                              double tolerance, int32_t maxIter, double* diffusiveFlux, double* Ynew, double info[3]);
int qgd_species_step_implicit_dev(qgd_device_t d, const double* Y, const double* Yb, const uint8_t* fixedValueFace, const double* rhoOld,
                                  const double* rho, const double* phiJmY, const double* muf, double Sc, double deltaT, const double* Su,
                                  double tolerance, int32_t maxIter, double* diffusiveFlux, double* Ynew, double info[3]);   /* device pointers */

/* QHDFoam's pressure equation -- QHDpEqn_8H_source.html L35-47:
 *     fvScalarMatrix pEqn(fvc::div(phiu) - fvc::div(phiwo) - fvm::laplacian(taubyrhof, p));
 *     pEqn.setReference(pRefCell, pRefValue);  pEqn.solve();  phi = phiu - phiwo + pEqn.flux();
 * assembled and solved on the device: Gauss laplacian with the uncorrected surface-normal gradient (L0), a
 * Jacobi-preconditioned conjugate gradient with reproducible reductions, converged on OpenFOAM's normalised residual
 * sum|b-Ax|/normFactor < tolerance (or < relTol x initial), at most maxIter iterations.
 * phiu, phiwo, taubyrhof: nFaces.  patchKind[nPatches]: QGD_BC_ZEROGRADIENT, QGD_BC_FIXEDVALUE (values pb[nBoundaryFaces])
 * or QGD_BC_QGDFLUX = fixedGradient with gradb[nBoundaryFaces] (what qhdFluxFvPatchScalarField::updateCoeffs leaves in
 * gradient(), qhdFluxFvPatchScalarField_8C_source.html L159-208); constraint patches are skipped.
 * p[nCells]: initial guess in, solution out.  phi[nFaces] out.  info = {iterations, initial residual, final residual}.
 * The reference level is applied only when no patch is fixedValue (fvMatrix::setReference, L0); pRefCell < 0: never. */
typedef struct qgd_poisson_control {
    double tolerance, relTol;
    int32_t maxIter, pRefCell;
    double pRefValue;
} qgd_poisson_control;
int qgd_poisson_control_default(qgd_poisson_control* c);
int qgd_qhd_pressure(qgd_device_t d, const double* phiu, const double* phiwo, const double* taubyrhof,
                     const int32_t* patchKind, const double* pb, const double* gradb, const qgd_poisson_control* ctl,
                     double* p, double* phi, double info[3]);

/* ---- QHDFoam case resident on the device --------------------------------------------------------------------------- */
/* The loop body of QHDFoam [QHDFoam_8C_source.html L83-139], both branches of implicitDiffusion: updateFields.H,
 * updateFluxes.H, the pressure equation QHDpEqn.H L35-47 (conjugate gradients preconditioned by an aggregation multigrid
 * built once: the matrix does not change, QHDFoam never re-corrects its thermo inside the loop), QHDUEqn.H L36-84,
 * QHDTEqn.H L65-91, the reference level of p (L123-130).  Thermo: rhoConst + constTransport (uniform rho0, mu, Pr; the QHD
 * closures leave muQGD = alphauQGD = 0 [T0byGr_8C_source.html L62-72]), laminar; L0 discretisation assumed: Gauss linear
 * gradients, Gauss linear uncorrected laplacians, Euler ddt.  Sharded meshes: see "the QHD case on a cell-range shard" below. */
/* qgdFlux [QGDInterpolate_8H_source.html L76-105]: the flux's own divSchemes entry decides */
enum qgd_flux_scheme {
    QGD_FLUX_LINEAR = 0,   /* no entry (flux*psif) or `Gauss linear` (fvc::flux with linear weights: the same numbers) */
    QGD_FLUX_UPWIND = 1    /* `Gauss upwind`: psi_f = pos0(flux)*(psi_O - psi_N) + psi_N (L0: upwind::weights = pos0(faceFlux),
                              surfaceInterpolationScheme::interpolate), patch faces keep the patch value               */
};

typedef struct qgd_qhd_options {
    int32_t stencil;          /* QGD_FVSC_*                                                                    */
    int32_t implicitDiffusion;/* 0: fvc::laplacian in both equations; 1 (the reference's default, QGDThermo_8C_source.html L70-82):
                                 fvm::laplacian(muf/rhof, U) and fvm::laplacian(Hif, T) [QHDUEqn_8H_source.html L46-65,
                                 QHDTEqn_8H_source.html L69-80]: the four systems as ONE matrix walk (see implicitTol)     */
    int32_t tauModel;         /* QGDCoeffs closure: 0 constTau (Tau), 1 HbyUQHD (aQGD, UQHD), 2 T0byGr (T0, Gr),
                                 3 H2bynuQHD (aQGD; nu = mu/rho0)                                                */
    int32_t pRefCell;         /* fvSolution pRefCell; < 0: no reference level                                  */
    int32_t pMaxIter;
    int32_t precond;          /* 1 aggregation multigrid (default), 0 Jacobi                                    */
    double rho0, mu, Pr, beta, g[3], deltaT;
    double Tau, aQGD, UQHD, T0, Gr;
    double pTol, pRelTol, pRefValue;
    double implicitTol;       /* implicitDiffusion: tolerance (OpenFOAM's normalised residual) of the U and T solves (1e-10) */
    int32_t implicitMaxIter;  /* ... and their iteration limit (1000)                                          */
    int32_t fluxSchemeU;      /* QGD_FLUX_* of qgdFlux(phi,U,Uf) [QHDUEqn_8H_source.html L41], entry `div(phi,U)`          */
    int32_t fluxSchemeT;      /* ... of qgdFlux(phi,T,Tf) [QHDTEqn_8H_source.html L65], entry `div(phi,T)`                 */
    int32_t pad_;
} qgd_qhd_options;
typedef struct qgd_qhd_case_s* qgd_qhd_case_t;
int qgd_qhd_options_default(qgd_qhd_options* opt);
int qgd_qhd_case_create(qgd_device_t d, const qgd_qhd_options* opt, qgd_qhd_case_t* out);
int qgd_qhd_case_free(qgd_qhd_case_t c);
/* per patch: U zeroGradient | fixedValue | slip; T zeroGradient | fixedValue; p zeroGradient | fixedValue (valueP) |
 * QGD_BC_QGDFLUX = fixedGradient with gradient valueP (what qhdFlux is inside QHDFoam) | QGD_BC_QHDFLUX (see the enum) */
int qgd_qhd_case_set_bc(qgd_qhd_case_t c, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT,
                        int32_t bcP, double valueP);
int qgd_qhd_case_set_fields(qgd_qhd_case_t c, const double* U, const double* T, const double* p);
int qgd_qhd_case_step(qgd_qhd_case_t c, int32_t nSteps);
/* "U","T","p" (+ ".boundary"), face fields "phi","phiu","phiwo","tauQGDf","hQGDf", "faceTerms" (4 nF, after a step: see the QHD run monitor) */
int qgd_qhd_case_get_field(qgd_qhd_case_t c, const char* name, double* out, int64_t outDoubles);
/* info[0]=time, [1]=deltaT in force, [2..4]= iterations / initial / final normalised residual of the last pressure solve,
 * [5]=steps, [6]=multigrid levels, [7]=milliseconds of the last pressure solve */
int qgd_qhd_case_info(qgd_qhd_case_t c, double info[8]);
/* QGD_QHD_FUSED=1 (off by default: at 8 M cells the one launch takes what the three kernels take, profiles/r06_ab_qhd_fused_advance.txt):
 * the U and T equations of the explicit branch [QHDUEqn_8H L36-84, QHDTEqn_8H L65-91] -- vertex values of p, face pass 2, explicit Euler
 * update -- run as ONE launch on the cell blocks of QGDFoam's one-launch step (qgd_qhd.hip qhdFusedAdvanceKernel).  info[0] = bit 0: they do
 * (bit 1 is reserved for the part in front of the pressure equation, not built); info[1] = blocks; info[2] = LDS bytes per workgroup;
 * info[3] = 0.  Needs a device with block tables (qgd_device_create, or _with QGD_DEVICE_FUSED_ANY_BLOCKS), 3-D GaussVolPoint, an unsharded
 * mesh, implicitDiffusion false; everything else keeps the separate kernels. */
int qgd_qhd_case_fused_info(qgd_qhd_case_t c, int64_t info[4]);
/* implicitDiffusion: the solve of the last step -- info[0..3] = iterations of Ux, Uy, Uz, T, [4..7] = initial, [8..11] = final
 * normalised residuals (what OpenFOAM prints as "Solving for Ux, Initial residual = ..."), [12] = steps since
 * qgd_qhd_case_set_fields in which a component stopped above implicitTol, [13] = 0 explicit branch | 1 conjugate gradients
 * (QGD_IMPL_SOLVER=pcg) | 2 Chebyshev iteration (default), [14] = steps in which a component ended at the rounding floor of its
 * true residual ABOVE implicitTol (see qgd_case_implicit_info), [15] reserved.  The four systems share |Sf| delta_f up to
 * {nu, nu, nu, Hi} and are solved as four right-hand sides of one matrix walk. */
int qgd_qhd_case_implicit_info(qgd_qhd_case_t c, double info[16]);

/* ---- SRFQHDFoam: the QHD case in a single rotating frame ----------------------------------------------------------------------
 * SRFQHDFoam.C L93-147 is QHDFoam's loop with two differences: the body force carries the Coriolis term,
 * BdFrc = beta*T*g - 2 (omega ^ Urel) [SRFQHDFoam/updateFields.H L73-74], and QHDTEqn.H is not included -- T stays as read.  The
 * velocity of the case is the RELATIVE one (the file Urel, createFields.H L22-33).  There is NO centrifugal term, as in the listing:
 * p is the reduced pressure (it carries the centrifugal potential).  gradWf (updateFields.H L45) is not formed: nothing reads it.
 *
 * qgd_qhd_case_set_srf: after qgd_qhd_case_create and before the first qgd_qhd_case_set_fields (later: QGD_ERR_INVALID).  omega in
 * rad/s.  flags = 0 is SRFQHDFoam's own loop: T, T.boundary are never written by a step, the implicitDiffusion branch solves three
 * systems (qgd_qhd_case_implicit_info reports 0 iterations for T).  QGD_SRF_SOLVE_T keeps QHDTEqn.H beside the Coriolis force: an
 * EXTENSION, not the reference's solver.  omega = (0,0,0) with QGD_SRF_SOLVE_T is the plain QHDFoam case, bit for bit.
 * A rotating or frozen-T case runs the separate kernels whatever QGD_QHD_FUSED says (qgd_qhd_case_fused_info bit 0 reads 0).
 * Refused: a sharded device (QGD_ERR_NOT_IMPLEMENTED); non-finite omega, a 1-D mesh, a mesh with one empty direction and omega not
 * parallel to it -- OpenFOAM does not solve the component along an empty direction, the force would be dropped (QGD_ERR_INVALID). */
#define QGD_SRF_SOLVE_T 1
int qgd_qhd_case_set_srf(qgd_qhd_case_t c, const double omega[3], int32_t flags);
/* info[0..2] = omega, [3] = 1 rotating (omega != 0), [4] = 1 T frozen, [5..7] = 0 */
int qgd_qhd_case_srf_info(qgd_qhd_case_t c, double info[8]);
/* One velocity per face of a fixedValue patch (3 per face, in the patch's face order) -- what a stationary wall is in the rotating
 * frame, SRFVelocity with `relative no`: Urel_b = inletValue - omega ^ (Cf - origin).  The contract of qgd_case_set_bc_values: the
 * patch's U entry must be fixedValue and nFaces the patch's size (else QGD_ERR_INVALID), U = NULL or a later qgd_qhd_case_set_bc of
 * the patch returns it to its one value, qgd_qhd_case_set_fields follows.  Independent of qgd_qhd_case_set_srf.
 * These three entries were added without a change of QGD_ABI_VERSION (it stays 9: no struct grew, no existing entry changed its
 * meaning). */
int qgd_qhd_case_set_bc_values(qgd_qhd_case_t c, int32_t patch, const double* U, int64_t nFaces);

/* ---- adjustTimeStep of QHDFoam and SRFQHDFoam ---------------------------------------------------------------------------------
 * QHDFoam.C L104-106 / SRFQHDFoam.C L114-116: readTimeControls.H, QHDCourantNo.H, setDeltaT-QGDQHD.H between updateFluxes.H and
 * runTime++.  With the control on, every qgd_qhd_case_step reduces on the device, after the fluxes of the step,
 *   M = max_f |phiu_f| / (|Sf_f| hQGDf_f)    [QHDCourantNo.H L44-48: Cof = deltaT |Uf & Sf/|Sf|| / hQGDf; phiu = Sf & Uf]
 * over every face that carries a field (internal and patch faces, not those of empty patches), and the host applies
 *   CoNum = deltaT M;  f = maxCo/(CoNum + SMALL);  deltaTFact = min(min(f, 1 + 0.1 f), 1.2)           [setDeltaT-QGDQHD.H L41-50]
 *   deltaT = min(deltaTFact deltaT, min(maxDeltaT, cTau min_f tauQGDf))                                 [L52-61]
 * (SMALL = 1e-15; min tauQGDf over the same faces, reduced once per qgd_qhd_case_set_fields: thermo is not corrected in the loop).
 * The pressure equation does not hold deltaT; the U and T equations of the step use the new one (Euler ddt; under implicitDiffusion
 * the diagonals V/deltaT + ... are rebuilt when deltaT differs from the one they were built with).  The pair is read at the one wait
 * a step has anyway (before the pressure solve): no further wait.  The start values of the solves (QGD_QHD_PEXTRAP,
 * QGD_IMPL_XEXTRAP) take the Lagrange weights of the actual step lengths, by value, whenever the steps behind them are unequal
 * (QGD_QHD_LAGRANGE=0: the equal-step weights whatever the steps); with equal steps the kernels and weights are those of a fixed deltaT,
 * bit for bit.  They move iteration counts only.  The face weights (8 B per face) and min tauQGDf are formed when the controls or
 * qgd_qhd_case_time_info are first asked for after qgd_qhd_case_set_fields: a case that never asks holds and launches nothing for them.
 *
 * qgd_qhd_case_set_time_control: any time between steps (readTimeControls.H is re-read on every pass), acts from the next step, and
 * survives qgd_qhd_case_set_fields (which returns deltaT to the options').  adjustTimeStep = 0 restores the options' fixed deltaT.
 * QGD_ERR_INVALID: maxCo, maxDeltaT or cTau non-finite or not positive (the listing's defaults: 1, GREAT, 0.75).
 * QGD_ERR_NOT_IMPLEMENTED: a sharded device (the maximum would need a MAX all-reduce point in the phase table).  With the control on,
 * qgd_qhd_case_step_phase and qgd_qhd_case_step_sharded return QGD_ERR_NOT_IMPLEMENTED: qgd_qhd_case_step alone serves it.
 *
 * qgd_qhd_case_time_info: info = {time, the deltaT in force (that of the last step, or after adjustTimeStep = 0 the options' again), CoNum the last step's control saw (deltaT before it x M), M of the last
 * step, min tauQGDf, adjustTimeStep, steps, 0}.  With the control off CoNum and M are still reported (reduced when asked for, from the
 * fluxes of the last step: a step of a case without the control launches nothing for it); both are 0 before the first step.
 * qgd_qhd_case_info[1] and the QHD run monitor's deltaT report the deltaT in force; time accumulates the adjusted steps;
 * qgd_qhd_case_get_field answers "hQGDf" (nF).  Added without a change of QGD_ABI_VERSION (it stays 9: no struct grew, no existing
 * entry changed its meaning). */
int qgd_qhd_case_set_time_control(qgd_qhd_case_t c, int32_t adjustTimeStep, double maxCo, double maxDeltaT, double cTau);
int qgd_qhd_case_time_info(qgd_qhd_case_t c, double info[8]);

/* ---- the QHD case on a cell-range shard (qgd_mesh_box slabs, qgd_mesh_shard) ------------------------------------------------
 * What the reference does through processor patches inside fvm::laplacian / PCG / fvc::grad under MPI
 * [QHDpEqn_8H_source.html L35-47, QHDUEqn_8H_source.html L36-84] becomes, per step, with ONE rank per shard:
 *   phase 0   flux assembly (updateFields.H, updateFluxes.H), p's boundary conditions, fvc::grad(U) of the owned cells, the rows
 *             of the pressure equation of the owned cells, first residual   -> DRAIN PENDING; all-reduce (SUM) control[0..3)
 *   phase 1   normFactor                                        -> all-reduce control[3]
 *   phase 2   first preconditioned residual, search direction   -> DRAIN PENDING; all-reduce control[4]; exchange message kind 2
 *   repeat until qgd_qhd_case_solve_status says done (every rank sees the same flag: it is computed from reduced sums):
 *     phase 3 A d, d.Ad                                         -> all-reduce control[5]
 *     phase 4 x, r, z = M r, |r|, r.z                            -> DRAIN PENDING; all-reduce control[6..8)
 *     phase 5 residual, iteration count, done?, new direction   -> exchange message kind 2
 *   phase 6   p's boundary conditions after the solve           -> exchange message kind 1
 *   phase 7   phi, QHDUEqn.H, QHDTEqn.H, U/T boundary conditions -> all-reduce control[8] (only when p needs a reference level)
 *             implicitDiffusion: phi, the face terms without the laplacians, the right-hand sides of the four systems; then the
 *             solve with ITS OWN 68-double control block (qgd_qhd_case_implicit_control*), phases and reductions exactly those of
 *             "the implicitDiffusion branch on a cell-range shard" below, numbered 10..15 here instead of 22..27, message kind 4 in
 *             place of its kind 3 (no start-value message: the ghost columns start from the state message), until
 *             qgd_qhd_case_implicit_solve_status says done; then
 *   phase 16  (implicitDiffusion) the solution into the records, U/T boundary conditions -> all-reduce control[8] as after phase 7
 *   phase 8   reference level of p                              -> exchange message kind 0
 * DRAIN PENDING = the comm points of the preconditioner, which fall INSIDE phases 0, 2 and 4: after the phase call, and again after
 * every qgd_qhd_case_step_phase(c, 9), ask qgd_qhd_case_pending and perform what it names until it answers 0 (protocol below).  A
 * caller that implements only the table and never drains gets an error status from the next phase ("a collective of the phase in
 * flight is pending"), not a wrong answer.
 * Preconditioner: by DEFAULT the smoothed-aggregation hierarchy SPANS THE RANKS (level 0 distributed, coarse levels replicated;
 * same iteration count as the unsharded solve).  It replicates the global matrix on every rank at set-up, so it is built only up
 * to QGD_MG_DIST_MAX_CELLS cells of the unsharded mesh (default 20 000 000; memory per rank ~ nCells (1 + 2K) doubles on host and
 * device, K = couplings per cell to higher-numbered neighbours, plus a host coarsening of nCells rows).  Above that, with
 * QGD_MG_DIST=0, with the plain-aggregation or double-precision cycle, or for a caller that never performs the set-up all-reduces,
 * every rank preconditions with the hierarchy of its own rows (block Jacobi across the shards: couplings to ghost cells stay in the
 * diagonal; 7 -> 65 / 97 / 140 iterations on 2 / 4 / 8 shards of a 128^3 box) and a line on stderr says so.  Everything else is the
 * unsharded arithmetic.
 * control: 16 device doubles (qgd_qhd_case_control_ptr); message kinds: 0 = the new state, {U,T} per cell (4) and per patch face
 * (4); 1 = p + fvc::grad(U) per cell (1 + 9: a ghost cell's gradient cannot be formed locally, it lacks faces) and p's patch value
 * + gradient per patch face (2); 2 = the search direction per cell (1); 3 = the multigrid iterate per cell (1), see qgd_qhd_case_pending;
 * 4 = what the implicitDiffusion solve's next matrix product reads in the ghost columns, {Ux, Uy, Uz, T} per cell (4).
 * pRefCell is a cell label of the UNSHARDED mesh.  All entries are stream-ordered on the device's stream. */
int qgd_qhd_case_step_phase(qgd_qhd_case_t c, int phase);
/* The hierarchy that spans the ranks (default up to QGD_MG_DIST_MAX_CELLS, see above).  Level 0 stays distributed --
 * each rank smooths its own rows, the ghost entries of the iterate refreshed before every sweep (message kind 3: one double per cell)
 * -- and every level below it is replicated: the ranks all-reduce their shares of the level-1 right-hand side and run the coarse part
 * of the cycle redundantly.  The comm points fall INSIDE phases 0 (set-up, first step only: the global matrix is gathered by two
 * all-reduces), 2 and 4 (the cycle), so after EVERY qgd_qhd_case_step_phase call the caller asks
 *     qgd_qhd_case_pending(c, &action, &ptr, &count)
 * and, while action != 0, performs it and calls qgd_qhd_case_step_phase(c, 9):
 *     action 1  exchange message kind 3 (halo_pack / halo_unpack with kind 3)
 *     action 2  SUM all-reduce of the `count` device doubles at ptr, in place
 *     action 3  MAX all-reduce of the same
 * then goes on with the reductions and messages the table above lists for that phase.  Every rank sees the same sequence.
 * qgd_qhd_case_step_sharded does all of this itself. */
int qgd_qhd_case_pending(qgd_qhd_case_t c, int32_t* action, void** devicePtr, int64_t* count);
/* the control block of the implicitDiffusion solve (68 doubles, control[slot * 4 + component], as qgd_case_implicit_control) and
 * its state: status[0] != 0: every component is done; status[1] = right-hand sides (4) */
int qgd_qhd_case_implicit_control(qgd_qhd_case_t c, double control[68], int set);
int qgd_qhd_case_implicit_control_ptr(qgd_qhd_case_t c, void** devicePtr);
int qgd_qhd_case_implicit_solve_status(qgd_qhd_case_t c, double status[2]);
int qgd_qhd_case_control_ptr(qgd_qhd_case_t c, void** devicePtr);
/* host copy of the control block out (set == 0) or in (set != 0), after everything queued so far: for transports that reduce on
 * the host (MPI_Allreduce of 16 doubles, torch.distributed over gloo) */
int qgd_qhd_case_control(qgd_qhd_case_t c, double control[16], int set);
/* waits for the stream; status = {done (0 no, 1 converged or out of iterations, 2 breakdown), iterations, initial, final residual} */
int qgd_qhd_case_solve_status(qgd_qhd_case_t c, double status[4]);
int qgd_qhd_case_sync(qgd_qhd_case_t c);
/* measurement: `reps` smoothing sweeps of multigrid level 0 (the kernel the pressure solve spends most of its time in) between two
 * HIP events; info = {average ms per sweep, rows, ELL width, bytes per matrix value and vector entry (4: single-precision cycle)} */
int qgd_qhd_case_sweep_time(qgd_qhd_case_t c, int reps, double info[4]);
/* The pressure preconditioner z = M r (one multigrid V-cycle) as an observable operator: three entries for tests, none of which
 * changes a solve.  QGD_ERR_INVALID before qgd_qhd_case_set_fields; QGD_ERR_NOT_IMPLEMENTED on a sharded device, with precond = 0
 * and for the hierarchy that spans the ranks.
 * mg_info: info[0..32) = {levels, single-precision cycle, smoothed aggregation, omega, oc, nu, nu0, coarseSweeps, cr[8], cm[8],
 *   fused hand-over possible (mode 1 of mg_apply), rows per r.z partial, QGD_MG_PT_ELL_MIN, 0...}, then 8 per level: {rows, layout
 *   (0 sliced ELL, 1 CSR rows), dense inverse, smoothed prolongator, P^T sliced, smootherScale, widest row, stored entries};
 *   cap >= 32 + 8 levels (128 always suffices).
 * mg_get: one array of one level copied BACK FROM DEVICE MEMORY (lengths from the start arrays read back, not from the builder's
 *   host copies); *n = its elements, buf == NULL: size query, 0: the level has no such array.  what: 0 diag, 1 sliceStart / rowStart,
 *   2 col, 3 val, 4 pS, 5 pCol, 6 pVal, 7 ptS, 8 ptCol, 9 ptVal, 10 agg, 11 aggStart, 12 aggItems, 13 inverse, 14 / 15 diag / val of
 *   the double-precision level.  Elements: int32_t (1, 2, 4, 5, 7, 8, 10, 11, 12), double (14, 15), otherwise the cycle's precision
 *   (float for a single-precision cycle, else double); cap counts elements.  Sliced ELL: entry k of row i at
 *   (sliceStart[i >> 6] + k) * 64 + (i & 63), col < 0 = padding; val holds a_ij = -A_ij, diag A_ii.
 * mg_apply: z = M r for host vectors over the rows (cells), through the solver's own preconditioner call.  mode 0: the separate
 *   passes; mode 1: the fused tail (the last level-0 sweep writes z in double and the partial sums of r.z per block of info[25]
 *   rows into rzPart, ceil(rows / info[25]) doubles; QGD_ERR_INVALID when info[24] == 0).  Runs with the control block's "done"
 *   flag cleared and puts the control block, r and z back as it found them. */
int qgd_qhd_case_mg_info(qgd_qhd_case_t c, double* info, int32_t cap);
int qgd_qhd_case_mg_get(qgd_qhd_case_t c, int32_t level, int32_t what, void* buf, int64_t cap, int64_t* n);
int qgd_qhd_case_mg_apply(qgd_qhd_case_t c, const double* r, double* z, int32_t mode, double* rzPart);
int qgd_qhd_case_halo_count(qgd_qhd_case_t c, int slot, int kind, int64_t* sendCount, int64_t* recvCount);
int qgd_qhd_case_halo_pack(qgd_qhd_case_t c, int slot, int kind, double* sendBufDevice);
int qgd_qhd_case_halo_unpack(qgd_qhd_case_t c, int slot, int kind, const double* recvBufDevice);

/* ---- scalarTransportQHDFoam case resident on the device ---------------------------------------------------------------- */
/* The loop body of scalarTransportQHDFoam [scalarTransportQHDFoam_8C_source.html L86-125]: U is read and never advanced, thermo.correct()
 * runs once, so Uf, phiu, tauQGDf, hQGDf and Hif = alphaf/rhof are constants of the run; per step gradTf = fvsc::grad(T), Tf =
 * qgdInterpolate(T), phiTf = qgdFlux(phiu,T,Tf), phiTauTReg = tauQGDf phiu (Uf & gradTf) and, ONLY with implicitDiffusion,
 *   solve(fvm::ddt(T) + fvc::div(phiTf) - fvc::Sp(fvc::div(phiu),T) - fvm::laplacian(Hif,T) - fvc::div(phiTauTReg) == TSu), TSu = 0.
 * The listing has no else: with implicitDiffusion 0 T stays as it is and only time advances (reproduced as listed).  Thermo and L0
 * discretisation are the QHDFoam case's (rhoConst + constTransport, uniform rho0, mu, Pr; Euler, Gauss linear uncorrected).  The solve is
 * the implicitDiffusion solver of the other cases (Chebyshev, QGD_IMPL_SOLVER=pcg: conjugate gradients), started from the old T.
 * adjustTimeStep [setDeltaT-QGDQHD_8H L41-61]: CoNum = deltaT max(|Uf|/hQGDf), deltaTFact = min(min(maxCo/(CoNum + SMALL),
 * 1 + 0.1 maxCo/(CoNum + SMALL)), 1.2), deltaT = min(deltaTFact deltaT, min(maxDeltaT, cTau min(tauQGDf))); both extrema are constants of
 * the run (reduced once on the device by qgd_scalar_case_set_fields), so a step waits for nothing.
 * One device: a sharded or periodic (qgd_mesh_unroll_cyclic) device is refused with QGD_ERR_NOT_IMPLEMENTED. */
typedef struct qgd_scalar_options {
    int32_t stencil;          /* QGD_FVSC_*                                                                    */
    int32_t implicitDiffusion;/* 1 (the reference's default): the T equation is solved; 0: T is left unchanged, as listed */
    int32_t tauModel;         /* 0 constTau (Tau), 1 HbyUQHD (aQGD, UQHD), 2 T0byGr (T0, Gr), 3 H2bynuQHD (aQGD; nu = mu/rho0) */
    int32_t adjustTimeStep;
    int32_t fluxSchemeT;      /* QGD_FLUX_* of qgdFlux(phiu,T,Tf) [.C L110], entry `div(phiu,T)`                 */
    int32_t implicitMaxIter;  /* iteration limit of the T solve (1000)                                         */
    double rho0, mu, Pr, deltaT;
    double Tau, aQGD, UQHD, T0, Gr;
    double maxCo, maxDeltaT, cTau;   /* controlDict maxCo, maxDeltaT; cTau (default 0.75)                       */
    double implicitTol;       /* tolerance (OpenFOAM's normalised residual) of the T solve (1e-10)             */
} qgd_scalar_options;
typedef struct qgd_scalar_case_s* qgd_scalar_case_t;
int qgd_scalar_options_default(qgd_scalar_options* opt);
int qgd_scalar_case_create(qgd_device_t d, const qgd_scalar_options* opt, qgd_scalar_case_t* out);
int qgd_scalar_case_free(qgd_scalar_case_t c);
/* per patch: U zeroGradient | fixedValue (valueU) | slip; T zeroGradient | fixedValue (valueT); symmetryPlane / symmetry / empty patches
 * keep their own field types whatever is asked for, as in the QHDFoam case */
int qgd_scalar_case_set_bc(qgd_scalar_case_t c, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT);
/* U (3 nCells), T (nCells): forms everything that does not depend on T and resets time, steps and the solver statistics */
int qgd_scalar_case_set_fields(qgd_scalar_case_t c, const double* U, const double* T);
int qgd_scalar_case_step(qgd_scalar_case_t c, int32_t nSteps);
/* "T", "T.boundary"; face fields (nFaces) "phiu", "tauQGDf", "hQGDf", "Uf" (3 per face), and, evaluated on the CURRENT T (what the next
 * step's updateFields.H would form), "gradTf" (3 per face), "phiTf", "phiTauTReg" */
int qgd_scalar_case_get_field(qgd_scalar_case_t c, const char* name, double* out, int64_t outDoubles);
/* info[0]=time, [1]=deltaT of the last step, [2]=CoNum the last step's time-step control saw (deltaT BEFORE it, times max(|Uf|/hQGDf);
 * fixed deltaT: that deltaT), [3]=steps, [4..6]= iterations / initial / final normalised residual of the last T solve, [7]=steps since
 * set_fields in which the solve stopped above implicitTol, [8]=steps in which a Chebyshev solve ended at the rounding floor of its
 * residual above implicitTol, [9]=0 no solve | 1 conjugate gradients | 2 Chebyshev, [10]=max(|Uf|/hQGDf), [11]=min(tauQGDf) */
int qgd_scalar_case_info(qgd_scalar_case_t c, double info[12]);
int qgd_scalar_case_sync(qgd_scalar_case_t c);

/* ---- QGDFoam case ----------------------------------------------------------- */

typedef struct qgd_case_options {
    int32_t stencil;          /* QGD_FVSC_* : fvSchemes fvsc{default ...;}        */
    int32_t implicitDiffusion;/* 0: the explicit branch [QGDFoam_2updateFluxes_8H_source.html L95-106];
                                 1: the reference's default [QGDThermo_8C_source.html L70-82]: viscous stress and heat
                                 conduction implicit, tauMC / phiSigmaDotU [updateFluxes.H L107-111, QGDUEqn_8H L54-75,
                                 QGDEEqn_8H L53-64]; on shards see "the implicitDiffusion branch on a cell-range shard"   */
    int32_t adjustTimeStep;   /* 1: Courant/deltaT control
                                 [QGDCourantNo_8H_source.html L36-53,
                                  setDeltaT-QGDQHD_8H_source.html L41-61]         */
    int32_t consistentEnergy; /* 0: the explicit energy re-solve as the listing has it, fvm::ddt(rho,e) - fvc::ddt(rhoE)
                                 [QGDEEqn_8H_source.html L67-72]: rho*e advances by the increment of rhoE and never gives
                                 the kinetic energy back (Sod's plateau comes out at p* = 0.330 instead of 0.303);
                                 1: keep e = rhoE/rho - |U|^2/2 of L49 (what the implicit branch's fvc::ddt(rho,e) form,
                                 L57, gives with a zero source): the physically consistent update                  */
    double R;                 /* perfectGas: specific gas constant                */
    double Cv;                /* eConst (Tref = 0, Esref = 0)                     */
    double mu;                /* constTransport: mu                               */
    double Pr;                /* constTransport: Pr                               */
    double ScQGD;             /* constScPrModel1 [constScPrModel1_8C_source.html L58-89] */
    double PrQGD;
    double alphaQGD;          /* uniform alphaQGD (0.5 when the file is absent
                                 [QGDCoeffs_8C_source.html L145-159])             */
    double deltaT;            /* (initial) time step                              */
    double maxCo, maxDeltaT, cTau; /* used when adjustTimeStep                    */
    double implicitTol;       /* implicitDiffusion: tolerance (OpenFOAM's normalised residual) of the U and e solves,
                                 fvSolution's `tolerance` of those fields                                         */
    int32_t implicitMaxIter;  /* ... and their iteration limit                                                    */
    int32_t fluxSchemeU;      /* QGD_FLUX_*: what qgdFlux(phiJm,U,Uf) [QGDFoam_2updateFluxes_8H_source.html L78] does: LINEAR = flux*psif,
                                 the default branch and `divSchemes{div(phiJm,U) Gauss linear;}` (same numbers); UPWIND =
                                 `div(phiJm,U) Gauss upwind;` -> fvc::flux [QGDInterpolate_8H_source.html L86-104]: the upwind cell's
                                 U on internal faces, the patch value on patch faces                                  */
    int32_t fluxSchemeH;      /* the same for qgdFlux(phiJm,H,Hf) [updateFluxes.H L119], entry `div(phiJm,H)`          */
    int32_t pad_;
    int32_t termStencil[4];   /* per-term entries of fvSchemes.fvsc [fvsc_8C_source.html L51-58] for the four face gradients of the step,
                                 in the order grad(U), grad(e), grad(rho), grad(p) [QGDFoam_2updateFluxes_8H_source.html L41-65]:
                                 0 = no entry of its own (the `default` word = `stencil`), else 1 + QGD_FVSC_*.  At most two distinct
                                 stencils per case (QGD_ERR_NOT_IMPLEMENTED beyond); a mixed case walks its faces through the generic
                                 gather kernels (each gradient formed by its own stencil, the flux algebra unchanged), a uniform one
                                 through the fused kernels as before.  GaussVolPoint's re-evaluation of its input's boundary
                                 conditions [GaussVolPointStencil_8C_source.html L73] follows grad(p)'s word.                   */
} qgd_case_options;

int qgd_case_options_default(qgd_case_options* opt);

int qgd_case_create(qgd_device_t d, const qgd_case_options* opt, qgd_case_t* out);
int qgd_case_free(qgd_case_t c);

/* Boundary conditions, per patch.  value: 3 doubles for U, 1 for T and p
 * (uniform fixedValue); ignored for the other kinds. */
int qgd_case_set_bc(qgd_case_t c, int32_t patch, int32_t bcU, const double* valueU,
                    int32_t bcT, double valueT, int32_t bcP, double valueP);

/* Per-face values of a fixedValue entry (`value nonuniform List<...>`): field 0 = U (3 * nFaces doubles), 1 = T, 2 = p
 * (nFaces doubles), HOST pointers, in the patch's face order on THIS device's mesh -- nFaces is the patch's size there: on a
 * shard that includes the patch faces of ghost cells, on a mesh from qgd_mesh_unroll_cyclic the faces of the copies, which
 * follow the real ones.  (Such a face's record comes from its original with the halo message; its entry is read only by the
 * start-up evaluation of qgd_case_set_fields, so give it the original's value.)  Call after qgd_case_set_bc, which returns
 * the patch to its uniform values, and before qgd_case_set_fields.  values == NULL drops the list: the entry reads its
 * uniform value again.  Refused (QGD_ERR_INVALID, by name) when the field's entry on that patch is not QGD_BC_FIXEDVALUE,
 * when the patch is a constraint (empty / symmetryPlane / symmetry / wedge), halo or cyclic patch, and when nFaces is not
 * the patch's size.  Every kernel that evaluates a fixedValue face reads the list; the implicitDiffusion branch assembles
 * the U systems of a case with per-face velocities with its separate kernels (qgd_case_fused_info reports 0, not 2).
 * qgd_case_get_bc_values returns what the entry prescribes per face (the list, or the uniform value repeated);
 * isList (may be NULL) tells which. */
int qgd_case_set_bc_values(qgd_case_t c, int32_t patch, int32_t field, const double* values, int64_t nFaces);
int qgd_case_get_bc_values(qgd_case_t c, int32_t patch, int32_t field, double* values, int64_t nFaces, int32_t* isList);

/* Non-uniform alphaQGD / ScQGD: the READ_IF_PRESENT volScalarFields "alphaQGD" [QGDCoeffs_8C_source.html L119-160] and
 * "ScQGD" [constScPrModel1_8C_source.html L66-79] of the time directory, cell values (nCells) and patch values
 * (nBoundaryFaces) as the files' own boundary conditions evaluate them.  NULL keeps the uniform value of the options.
 * Call before qgd_case_set_fields. */
int qgd_case_set_qgd_coeffs(qgd_case_t c, const double* alphaQGD, const double* alphaQGDb, const double* ScQGD,
                            const double* ScQGDb);

/* The varScModel7 closure of QGDCoeffs [varScModel7_8C_source.html L166-300]: ScQGD of a cell is a shock sensor built from the
 * pressure jumps across the cell's faces,
 *     ScQGD = cSc1 |sum_f r_f (p_other - p_self)| / (sum_f p_f / n),   r_f = nonOrthDeltaCoeff_f / deltaCoeff_f,
 * over the internal faces (p_f = linear interpolate) and the patch faces (p_f = p_b) of the cell, those of empty patches left out;
 * then max(., minSc) where minSc >= 0, min(., maxSc) where maxSc >= 0, and ScQGD itself on the nConstCells cells of constCells
 * (the cellSet constScCellSet; labels of this device's mesh).  Patch faces keep ScQGD, clipped the same way.  tauQGD, tauQGDf and
 * alphauQGD are those of constScPrModel1; muQGD = p ScQGD tauQGD with the pressure of the step's start.  The sensor runs once in
 * qgd_case_set_fields and once per step, between the flux assembly and the advance, on every path of qgd_case_step /
 * qgd_case_step_phase / qgd_case_step_sharded, over the owned cells of a shard.
 * Call before qgd_case_set_fields.  opt == NULL returns the case to its uniform ScQGD (or the array of qgd_case_set_qgd_coeffs).
 * Refused: together with a ScQGD array of qgd_case_set_qgd_coeffs (alphaQGD arrays are allowed), on a periodic device
 * (qgd_mesh_unroll_cyclic), a model other than 7, a cell label out of range. */
typedef struct qgd_var_sc_options {
    int32_t model;       /* 7 */
    int32_t nConstCells;
    double ScQGD, cSc1, minSc, maxSc;   /* minSc, maxSc < 0: no clipping on that side */
} qgd_var_sc_options;
int qgd_case_set_var_sc(qgd_case_t c, const qgd_var_sc_options* opt, const int32_t* constCells);
/* out[0] = max, out[1] = min of ScQGD over the owned cells (the reference's "max/min ScQGD" line), computed when asked. */
int qgd_case_sc_range(qgd_case_t c, double out[2]);

/* Species mass fractions carried by the case: the species block of reactingLagrangianQGDFoam [reactingLagrangianQGDFoam_8C_source.html
 * L92-140].  Every qgd_case_step then advances nSpecies fields Y_i with the flow, in the reference's order: the species fluxes
 * [reactingLagrangianQGDFoam_2updateFluxes_8H_source.html L103-132], QGDRhoEqn, the species equations [QGDYEqn_8H_source.html L38-92:
 * the branch of the case's implicitDiffusion, L47-66 (the reference's default) or L67-86], QGDUEqn, QGDEEqn:
 *     phiJmY_i = phiJm Yf_i - phi tauQGDf (Uf & fvsc::grad(Y_i)),   ddt(rho Y_i) + div(phiJmY_i) - laplacian(muf / Sc_i, Y_i) = 0,
 *     Y_i.max(0),   Y_inert = max(1 - sum of the others, 0),
 * with the case's stencil (reduced, leastSquares 2-D, GaussVolPoint 2-D / 3-D) and the uncorrected snGrad in the laplacian.
 * The composition is PASSIVE: all species share the case's one `mixture` thermo; there is no chemistry (combustion->R), no parcel
 * source, and Y does not feed back into thermo.  Reacting thermo is out of scope.
 * The block reads the mass flux of every face, which the fused kernels never write: a case with species runs the three-kernel explicit
 * step (fixed or adjusted deltaT), or, with implicitDiffusion, the separate kernels of the implicit branch (the block-fused assembly of
 * the U systems keeps the internal faces' mass flux in its blocks) -- qgd_case_fused_info reports 0 after this call.
 * implicitDiffusion true, asked for with the flag QGD_SPECIES_IMPLICIT [QGDYEqn.H L47-66]: fvm::ddt(rho, Y_i) + fvc::div(phiJmY_i) - fvm::laplacian(muf / Sc_i, Y_i), solved inside the
 * implicit advance, after deltaT and before the U systems, on the old records.  All species share the face coefficient muf |Sf| delta_f
 * and differ by 1 / Sc_i: a register batch of species ([2] of qgd_case_species_info) is ONE solve of the case's implicit solver
 * (Chebyshev, or conjugate gradients with QGD_IMPL_SOLVER=pcg) with that many right-hand sides.  fixedValue patches of a species enter
 * its diagonal and source; diffusiveFlux_i += YEqn.flux() of the new Y_i, with the listing's sign (opposite to the explicit branch's).
 * The solves start from the old Y_i: the time-extrapolated start values of the flow's solves (QGD_IMPL_XEXTRAP) are not extended to them.
 * Legal after qgd_case_create and before qgd_case_set_fields (QGD_ERR_INVALID afterwards).  At most QGD_MAX_SPECIES species.
 * QGD_ERR_NOT_IMPLEMENTED, with the reason named: implicitDiffusion true without the flag QGD_SPECIES_IMPLICIT; a sharded device or
 * a periodic (qgd_mesh_unroll_cyclic) device without the flag QGD_SPECIES_HALO, or with it and implicitDiffusion true (the batched species
 * solves are not distributed); per-term stencils (qgd_case_options::termStencil).  QGD_ERR_INVALID: nSpecies < 2 or > QGD_MAX_SPECIES, inertIndex out of
 * range, a Schmidt number <= 0 (ScNumbers == NULL: all 1), unknown flags.  Not served: the fused blocks, reacting thermo.  Run monitors report the species through
 * qgd_monitor_enable_species (masses, extrema, probes, patch fluxes; below, with the monitors).
 * Cell-range shards and cyclic patches, asked for with the flag QGD_SPECIES_HALO, explicit branch: ghost cells then carry their originals'
 * composition.  The state message (kind 0: qgd_case_halo_count / _pack / _unpack, qgd_case_halo_exchange, qgd_case_step_sharded in both
 * orders, the self-exchange of a periodic device) grows from 8 to 8 + nSpecies doubles per cell: its front -- 8 per cell, 12 per patch
 * face -- is laid out as without species, the species follow as nSpecies planes of one double per cell of the slot's list (species-major,
 * the inert species included).  Patch values do not travel: the unpack re-evaluates those of the slot's ghost patch faces from each
 * species' boundary condition.  The species' cell and patch kernels then follow the cell roles of the flow's (ghosts are written by the
 * unpack alone; the boundary layer of a shard can go first, phases 10 / 11).
 * qgd_case_step_phase is refused on a case with species, except phases 0, 1, 2, 5, 6, 10, 11 of a case with QGD_SPECIES_HALO on a sharded
 * device; qgd_case_step (and qgd_case_step_sharded, and phases 0 / 5) with a species whose field was never set is QGD_ERR_INVALID.
 * QGD_SPECIES_HALO was added without a change of QGD_ABI_VERSION (it stays 9: no struct grew, no entry was added or changed its meaning;
 * a library without the flag answers it with QGD_ERR_INVALID "unknown flags").
 * These entries (the five of the explicit block, then qgd_case_set_species_solver and qgd_case_species_implicit_info) were added without a change of QGD_ABI_VERSION (no struct grew, no existing entry changed its meaning): a host that
 * must run against older builds of the library looks the symbols up (dlsym) instead of comparing the number. */
#define QGD_MAX_SPECIES 32
#define QGD_SPECIES_KEEP_FLUXES 1   /* flags: keep phiJmY_i and diffusiveFlux_i of the last step (qgd_case_get_species_field) */
#define QGD_SPECIES_IMPLICIT 2      /* flags: the caller accepts the implicitDiffusion branch of the species equations (a case created with
                                     * implicitDiffusion = 1).  Without it such a case is answered with QGD_ERR_NOT_IMPLEMENTED as before this
                                     * branch was served: a host that runs the stateless qgd_species_step_implicit loop on that answer keeps
                                     * working unchanged, and nobody gets linear solves inside the step without asking.  Ignored on the explicit branch. */
#define QGD_SPECIES_HALO 4          /* flags: the caller accepts species on a sharded or periodic device: the state message carries the
                                     * composition (8 + nSpecies doubles per cell; size the buffers by qgd_case_halo_count).  Without it such a
                                     * device is answered with QGD_ERR_NOT_IMPLEMENTED as before.  On an ordinary device it changes nothing. */
int qgd_case_set_species(qgd_case_t c, int32_t nSpecies, int32_t inertIndex, const double* ScNumbers, int32_t flags);
/* Boundary condition of one species on one patch: QGD_BC_ZEROGRADIENT (the default of generic patches), QGD_BC_FIXEDVALUE with one
 * value for the patch, QGD_BC_NONE; constraint patches keep QGD_BC_NONE (their faces carry no species flux, or a zero gradient). */
int qgd_case_set_species_bc(qgd_case_t c, int32_t species, int32_t patch, int32_t bc, double value);
/* Cell values of one species (nCells doubles, HOST); its patch values follow from its boundary conditions. */
int qgd_case_set_species_fields(qgd_case_t c, int32_t species, const double* Y);
/* "Y" (nCells), "Y.boundary" (nBoundaryFaces); with QGD_SPECIES_KEEP_FLUXES also "phiJmY" and "diffusiveFlux" (nFaces, by face label)
 * as the last step formed them: the inert species' phiJmY is zero, its diffusiveFlux minus the sum of the others' [QGDYEqn.H L83]. */
int qgd_case_get_species_field(qgd_case_t c, int32_t species, const char* name, double* out, int64_t outDoubles);
/* info[0] = nSpecies (0: the case carries none), [1] = inertIndex, [2] = species per register batch of the face and cell kernels,
 * [3] = 1 with QGD_SPECIES_KEEP_FLUXES */
int qgd_case_species_info(qgd_case_t c, int64_t info[4]);
/* Controls of the species' solves on the implicitDiffusion branch (fvSolution.solvers.<species>): tolerance > 0, maxIter >= 1, for all
 * species.  Without this call they are the case's implicitTol / implicitMaxIter.  QGD_ERR_INVALID on a case without species or on the
 * explicit branch. */
int qgd_case_set_species_solver(qgd_case_t c, double tolerance, int32_t maxIter);
/* Statistics of the species' solves, 3 + 3 nSpecies doubles (infoDoubles: what info holds): info[0] = steps in which a species' solve
 * stopped above its tolerance (iteration limit or breakdown), [1] = steps in which one ended at the rounding floor of its residual above
 * the tolerance -- the meanings of [12] and [14] of qgd_case_implicit_info --, [2] = nSpecies; then per species i, by its index:
 * [3 + 3 i] = iterations, [4 + 3 i] = initial and [5 + 3 i] = final normalised residual of the last step (the inert species: zeros).
 * Counted since qgd_case_set_fields.  Waits for the case's stream. */
int qgd_case_species_implicit_info(qgd_case_t c, double* info, int64_t infoDoubles);

/* Initial cell fields U (nCells*3), T, p (HOST pointers); evaluates the BCs,
 * thermo.correct() and the derived conserved fields like createFields.H
 * [QGDFoam_2createFields_8H_source.html L3-109]. */
int qgd_case_set_fields(qgd_case_t c, const double* U, const double* T,
                        const double* p);

/* updateFields.H + updateFluxes.H on the current state.  Afterwards the face
 * fields "phiJm","phiJmU","phiP","phiPi","phiJmH","phiQ","phiPiU","phiwStar",
 * "phi","tauQGDf" are readable with qgd_case_get_field (debug / BC coupling
 * path: it materialises them; qgd_case_step does not). */
int qgd_case_update_fluxes(qgd_case_t c);

/* nSteps passes of the QGDFoam loop body, fully device resident. */
int qgd_case_step(qgd_case_t c, int32_t nSteps);

/* Named field copy-out to HOST.  Cell fields: "rho","U","p","e","T","rhoU",
 * "rhoE","c","psi","mu","alphau","tauQGD","muQGD","alphauQGD","hQGD","H","ScQGD"
 * (the uniform value repeated, the array of qgd_case_set_qgd_coeffs, or the last result of the varScModel7 sensor).
 * Face fields: see qgd_case_update_fluxes plus "hQGDf"; with implicitDiffusion true also "phiTauMC" (3 per face)
 * and "phiSigmaDotU" as the last step formed them [QGDFoam_2updateFluxes_8H_source.html L107-111, QGDUEqn_8H_source.html L72-74].
 * Boundary fields: "<cellfield>.boundary".  outDoubles = capacity of out. */
int qgd_case_get_field(qgd_case_t c, const char* name, double* out,
                       int64_t outDoubles);

/* info[0]=time, [1]=deltaT, [2]=CoNum, [3]=min(rho), [4]=min(e), [5]=step count */
int qgd_case_info(qgd_case_t c, double info[6]);
/* Whether this case advances with the fused kernel of the explicit step (QGD_FUSED, default on): a uniform 3-D GaussVolPoint case, explicit
 * branch, fixed deltaT (linear or `Gauss upwind` qgdFlux schemes); shards included.  One workgroup per block of <= 128 cells then stages the records of those
 * cells and of the cells around them in LDS, forms the vertex values of the block from them (volPointInterpolation's weights, pointCells
 * order), computes every internal face of its cells into LDS and advances the cells from there, in the summation order of
 * fvc::surfaceIntegrate: neither the vertex values nor the net fluxes of internal faces reach device memory, and the vertex kernel, the face
 * kernel and the cell kernel are one launch.  Same arithmetic, bit-identical states.  info[0] = 1 when in use (2: the same blocks assemble
 * the three U systems of an unsharded fixed-deltaT implicitDiffusion case in one launch -- vertex values, QGD fluxes, tauMC, phiTauMC, the rows
 * [QGDUEqn_8H_source.html L36-68, QGDFoam_2updateFluxes_8H_source.html L95-111], QGD_IMPL_FUSED; 3: Courant-number control, adjustTimeStep
 * [QGDCourantNo_8H_source.html L36-53, setDeltaT-QGDQHD_8H_source.html L41-61] -- the blocks run up to their cells' flux sums and their faces'
 * Courant partials, deltaT follows on the device, a cell kernel advances: two launches, QGD_FUSED_ADJUST; 0: the separate kernels), [1] = blocks, [2] = internal
 * faces computed per step (faces on a block's surface are computed by the block on either side), [3] = LDS bytes per workgroup, [4] = cell
 * records staged per step over all blocks, [5] = of which with their second record and centre (own cells + cells across a face), [6] =
 * vertex values formed per step over all blocks, [7] = on a shard, the leading blocks that hold the cells a neighbouring rank waits for (phase 10
 * launches them, phase 11 the others; whole bricks, so they hold other owned cells too).  Owned cells / info[1] = mean cells per block: 128
 * on a box its bricks divide, 123 on a 50-plane slab between two cuts.  qgd_case_update_fluxes and every other branch keep the separate kernels. */
int qgd_case_fused_info(qgd_case_t c, int64_t info[8]);
/* The linear solves of the implicitDiffusion branch in the last step (what OpenFOAM prints as "Solving for Ux, Initial
 * residual = ..., Final residual = ..., No Iterations ...") [QGDUEqn_8H_source.html L54-68, QGDEEqn_8H_source.html L53-61]:
 * info[0..3] = iterations of Ux, Uy, Uz, e; [4..7] = initial, [8..11] = final normalised residuals; [12] = number of steps
 * since qgd_case_set_fields in which a solve stopped above implicitTol (iteration limit or breakdown: the step keeps the last
 * iterate, as OpenFOAM does, and counts here); [13] = 0 explicit branch | 1 implicit, conjugate gradients (QGD_IMPL_SOLVER=pcg) |
 * 2 implicit, Chebyshev iteration (the default).  The Chebyshev iteration measures the TRUE residual b - A x of its iterate (the
 * conjugate-gradient loop a recurrence); when that stops falling below 1e-8 -- the rounding floor of the product, which OpenFOAM's
 * normalisation can lift to 1e-12 on nearly uniform fields -- the component stops there and is NOT counted as unconverged in [12];
 * [14] = number of steps in which a solve ended that way ABOVE implicitTol (OpenFOAM would have iterated on to maxIter and printed the
 * residual: "solved to implicitTol" holds only while [12] and [14] are both 0); [15] reserved. */
int qgd_case_implicit_info(qgd_case_t c, double info[16]);
/* measurement: `reps` matrix products of the three-component U system (QGDUEqn_8H_source.html L54-68: the `fvm::laplacian(muf,U)`
 * matrix applied to a search direction; the kernel the branch spends most of its time in) between two HIP events, on the vectors
 * the last step left; info = {average ms per product, rows} */
int qgd_case_implicit_apply_time(qgd_case_t c, int reps, double info[2]);

/* ---- the implicitDiffusion branch on a cell-range shard -------------------------------------------------------------------------
 * implicitDiffusion true is the reference's default [QGDThermo_8C_source.html L70-82].  Its two implicit equations
 * [QGDUEqn_8H_source.html L54-75, QGDEEqn_8H_source.html L53-64] are solved here with the scalars of the solve in a control block
 * on the device (the three velocity components as three right-hand sides of ONE matrix walk).  The solver is a Chebyshev iteration
 * on the Jacobi-preconditioned system by default (these matrices are strictly diagonally dominant, Gershgorin bounds the spectrum;
 * no dot products), or Jacobi-preconditioned conjugate gradients with QGD_IMPL_SOLVER=pcg; the phases, reductions and messages below
 * serve both (a slot the algorithm in use does not write is zero, a phase it does not need does nothing).  Under MPI the reference
 * reaches across ranks through processor patches inside fvm::laplacian, the linear solver and fvc::grad.  With one rank per shard
 * the advance (after phase 0, the flux assembly) is, through qgd_case_step_phase:
 *   phase 20  deltaT, fvc::grad(U) of the old state          -> exchange message kind 1
 *   phase 21  tauMC / phiTauMC, rho, rhoU, the three U systems and their start values -> exchange kind 4
 *   phase 22  first solver phase (A x, r, row radii)          -> SUM-reduce control[0..12), MAX-reduce control[32..36)
 *   phase 23  normFactor                                      -> SUM-reduce control[12..16)
 *   phase 24  first residual; Chebyshev: x_1 | CG: search direction, r.z -> SUM-reduce control[16..20); exchange kind 3
 *   repeat until qgd_case_implicit_solve_status says done:
 *     phase 25 Chebyshev: one step, sum |b - A x| | CG: A d, d.Ad    -> SUM-reduce control[20..24)
 *     phase 26 Chebyshev: residual, done?, next constants | CG: x, r, |r|, r.z -> SUM-reduce control[24..32)
 *     phase 27 Chebyshev: nothing | CG: new direction           -> exchange kind 3
 *   phase 28  U into the records, its boundary conditions     -> exchange kind 2
 *   phase 29  fvc::grad(U) of the new velocity                -> exchange kind 1
 *   phase 30  phiSigmaDotU, the energy equation, the e system and its start value -> exchange kind 4; then 22, 23, 24, (25, 26, 27)*
 *   phase 35  rhoE, thermo, p, boundary refresh               -> the state message (qgd_case_halo_pack / unpack), phase 2
 * control: 68 device doubles, slot-major, control[slot * 4 + component].  Message kinds: 1 = fvc::grad(U), 9 per cell; 2 = U, 3 per
 * cell; 3 = what the next matrix product reads in the ghost columns (Chebyshev: the iterate, CG: the search direction), 4 = the start
 * value of the solve in flight, one per right-hand side per cell (counts report room for three).
 * An unsharded case runs the same phases back to back inside qgd_case_step; qgd_case_step_sharded drives them over RCCL. */
int qgd_case_implicit_halo_count(qgd_case_t c, int slot, int kind, int64_t* sendCount, int64_t* recvCount);
int qgd_case_implicit_halo_pack(qgd_case_t c, int slot, int kind, double* sendBufDevice);
int qgd_case_implicit_halo_unpack(qgd_case_t c, int slot, int kind, const double* recvBufDevice);
int qgd_case_implicit_control(qgd_case_t c, double control[68], int set);
int qgd_case_implicit_control_ptr(qgd_case_t c, void** devicePtr);
/* waits for the stream; status[0] != 0: every right-hand side of the solve in flight is done; status[1] = their number */
int qgd_case_implicit_solve_status(qgd_case_t c, double status[2]);

/* ---- halo exchange of ghost-cell primitives (multi-GPU) ------------------- */
/* A shard has one halo slot per neighbouring shard: a qgd_mesh_box slab (kLo>0 or kHi<nzGlobal) has slot 0 = lower k
 * and slot 1 = upper k; a qgd_mesh_shard mesh has one per rank in "haloPeer".  count / recv_count = number of doubles
 * in the message sent to / received from that neighbour.  pack gathers the owned boundary-layer cells' records into
 * the DEVICE buffer sendBuf; unpack scatters recvBuf into the ghost cells.
 * The state message carries 8 doubles per cell -- {rho, Ux, Uy, Uz, p, e} as SURVEY 8(e) plans, plus H and muQGD, the two derived
 * quantities a receiver cannot rebuild from them (rhoE is an independent field under the listing's energy re-solve; muQGD is formed with
 * the previous step's pressure and the owner's hQGD); c and alphaQGD/c are recomputed on arrival -- and 12 per patch face of those cells
 * (both records, the qgdFlux gradient, the lagged patch density).  Always ask qgd_case_halo_count: the layout may change.
 * Both are asynchronous on the case's stream; qgd_case_stream_sync waits. */
/* Plain device buffers for callers that own the transport (GPU-aware MPI, RCCL, ...). */
int qgd_device_alloc(qgd_device_t d, int64_t bytes, void** devicePtr);
int qgd_device_release(qgd_device_t d, void* devicePtr);
int qgd_case_halo_count(qgd_case_t c, int slot, int64_t* count);
int qgd_case_halo_recv_count(qgd_case_t c, int slot, int64_t* count);
int qgd_case_halo_pack(qgd_case_t c, int slot, double* sendBufDevice);
int qgd_case_halo_unpack(qgd_case_t c, int slot, const double* recvBufDevice);
int qgd_case_stream_sync(qgd_case_t c);
/* Run the case's kernels on a caller-owned HIP stream (hipStream_t passed as
 * void*), e.g. the stream the RCCL halo transfers are ordered on, so that
 * compute and exchange need no host synchronisation between them. */
int qgd_case_set_stream(qgd_case_t c, void* hipStream);
/* One step in two stream-ordered phases so that the exchanges between them are the caller's:
 *   phase 0 = flux assembly; with adjustTimeStep it leaves {max Cof, -min tauQGDf} of this shard in the
 *             2-double device buffer of qgd_case_reduction_ptr -- MAX-all-reduce it over the ranks in place
 *             [QGDCourantNo_8H L50, setDeltaT-QGDQHD_8H L46 are global reductions];
 *   phase 1 = deltaT, cell update, boundary refresh; then halo_pack / exchange / halo_unpack.
 * To overlap the exchange with the bulk of the cell update, phase 1 splits further:
 *   phase 10 = deltaT + update of the shard's boundary layer only (the cells a neighbour needs and their patch faces),
 *   phase 11 = update of all remaining owned cells and patch faces;
 * halo_pack may start as soon as phase 10 is done (on the halo stream of qgd_case_set_halo_stream, ordered after the
 * compute stream by the caller), phase 11 runs meanwhile, and the next phase 0 waits for halo_unpack.
 * Ghost cells and their patch faces are written by halo_unpack only.  phase 2 is a no-op hook.
 * phase 3 = one whole step of an UNSHARDED case, stream-ordered like the others (qgd_case_step without its host synchronisation; the
 *   fused face + cell kernel when qgd_case_fused_info says the case uses it).
 * Phase 0 itself splits when qgd_case_mid_exchange_needed says so (a shard whose GaussVolPoint stencil meets a wall with the qgdFlux
 * pressure condition): GaussVolPoint re-evaluates p's boundary conditions inside fvsc::grad(p) [GaussVolPointStencil_8C_source.html
 * L73 -> qgdFluxFvPatchScalarField_8C_source.html L184-192], a ghost cell's patch face forms that mid-step patch pressure from an
 * incomplete stencil, and the vertex values of p on the wall carry it into the stencil of owned faces (1e-7 in a few cells).  So
 *   phase 5 = the assembly up to and including that re-evaluation  -> exchange the mid message (qgd_case_mid_halo_*: 2 doubles per
 *             patch face of the boundary-layer cells)
 *   phase 6 = the rest of the assembly (+ the Courant reduction of phase 0).
 * What the reference gets from the processor-patch evaluation inside correctBoundaryConditions(). */
int qgd_case_step_phase(qgd_case_t c, int phase);
int qgd_case_mid_exchange_needed(qgd_case_t c, int32_t* needed);
int qgd_case_mid_halo_count(qgd_case_t c, int slot, int64_t* sendCount, int64_t* recvCount);   /* in doubles */
int qgd_case_mid_halo_pack(qgd_case_t c, int slot, double* sendBufDevice);
int qgd_case_mid_halo_unpack(qgd_case_t c, int slot, const double* recvBufDevice);
int qgd_case_reduction_ptr(qgd_case_t c, void** devicePtr);
/* Stream (hipStream_t as void*) the halo pack/unpack kernels run on; default: the case's compute stream. */
int qgd_case_set_halo_stream(qgd_case_t c, void* hipStream);

/* ---- native halo transport (RCCL over xGMI, inside the library) ------------------------------------------------------ */
/* For a C++/MPI host: what replaces the reference's per-gradient-call PstreamBuffers exchange
 * [extendedFaceStencilScalarGrad_8C_source.html L145-233] and the processor-patch evaluation behind
 * correctBoundaryConditions() [GaussVolPointStencil_8C_source.html L73] is ONE grouped ncclSend/ncclRecv pair per
 * neighbouring rank per step.  RCCL is bound at run time (an RCCL already loaded in the process is reused, otherwise
 * librccl.so of the ROCm installation; QGD_RCCL_LIB overrides); without it these entries return QGD_ERR_NOT_IMPLEMENTED
 * and the pack/unpack entries above remain for callers with their own transport (GPU-aware MPI, torch.distributed).
 * Bootstrap like NCCL's: rank 0 asks for the 128-byte unique id, the host broadcasts it (MPI_Bcast / Pstream), every rank
 * creates its communicator for its HIP device. */
typedef struct qgd_comm_s* qgd_comm_t;
int qgd_comm_unique_id(void* id128);
int qgd_comm_create(int deviceId, int rank, int nRanks, const void* id128, qgd_comm_t* out);
int qgd_comm_free(qgd_comm_t comm);
/* info = {this rank (ncclCommUserRank), ranks RCCL itself counts in the communicator (ncclCommCount), HIP device (ncclCommCuDevice)}:
 * what the transport SAW, for logs and bench lines -- not what the caller asked for */
int qgd_comm_info(qgd_comm_t comm, int32_t info[3]);
/* pack -> send/recv with peers[slot] (rank behind each halo slot; < 0: skip the slot) -> unpack, stream-ordered on the
 * case's stream, buffers owned by the library.  No-op for an unsharded case. */
int qgd_case_halo_exchange(qgd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots);
/* MAX all-reduce of the {max Cof, -min tauQGDf} device buffer between step phases 0 and 1 (adjustTimeStep)
 * [QGDCourantNo_8H_source.html L50, setDeltaT-QGDQHD_8H_source.html L46]; no-op on one rank */
int qgd_case_allreduce_max(qgd_case_t c, qgd_comm_t comm);
/* One step of a sharded case: assemble, (adjustTimeStep: all-reduce), advance, exchange.  overlapped != 0: the shard's
 * boundary layer is updated first and the exchange runs on the library's halo stream while the compute stream updates the
 * remaining cells; the next assembly waits for the unpack through an event.  Stream-ordered (qgd_case_stream_sync waits). */
int qgd_case_step_sharded(qgd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int overlapped);
/* The QHD case over the same transport: one message of kind 0 / 1 / 2 per neighbouring rank (after qgd_qhd_case_set_fields:
 * kind 0 once), and nSteps whole steps -- phases, ncclAllReduce of the control block, exchanges -- with no host wait except the
 * run-ahead check of the pressure solve (the host reads the "done" flag of iteration i-2 before it queues iteration i). */
int qgd_qhd_case_halo_exchange(qgd_qhd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int kind);
int qgd_qhd_case_step_sharded(qgd_qhd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int32_t nSteps);

/* ---- measurement ------------------------------------------------------------ */
/* Kernel ids for qgd_case_kernel_time. */
enum {
    QGD_K_POINT = 0,   /* cell -> vertex interpolation                          */
    QGD_K_FACE = 1,    /* fused internal-face gradient + flux kernel            */
    QGD_K_BFACE = 2,   /* boundary-face flux kernel                             */
    QGD_K_CELL = 3,    /* flux gather + Euler update + thermo + QGD coefficients */
    QGD_K_BC = 4,      /* boundary-condition refresh                            */
    QGD_K_BPOINT = 5,  /* patch points: mean of the surrounding patch-face values */
    QGD_K_VARSC = 6,   /* varScModel7: ScQGD from the pressure jumps (qgd_case_set_var_sc) */
    QGD_K_COUNT = 7
};
/* Enable HIP-event timing of every launch of kernel `k` on the case's own
 * stream; totals since the last reset. */
int qgd_case_timing(qgd_case_t c, int enable);
int qgd_case_kernel_time(qgd_case_t c, int k, double* totalMs, int64_t* launches);
int qgd_case_timing_reset(qgd_case_t c);
/* Bytes resident on the device for this case + its mesh. */
int qgd_case_device_bytes(qgd_case_t c, int64_t* bytes);

/* ---- run monitors of a QGDFoam case ------------------------------------------ */
/* A monitor is created once for a case with a specification (probe cells, patches) and sampled by a few launches and one small
 * copy on the case's stream: volume integrals over the owned cells, extrema with the cells they sit in, the count and first
 * label of non-finite cells, the probes' values and, per requested patch, the totals of the net face fluxes the cell update
 * consumes.  Sampling writes nothing to the case and changes none of its launches; the order of every sum depends on the mesh
 * and the specification only, so two samples of one state are bitwise equal.
 *
 * Result block (doubles; qgd_monitor_layout gives the offsets of its QGD_MONITOR_SECTIONS sections):
 *   0 header (8):    owned cells | flux state (0: no assembly yet, patch fluxes are NaN; 1: all five; 2: implicitDiffusion, where
 *                    flux[1..4] hold the explicit part only: mass is reported, the other four are NaN) | nProbes | nPatches |
 *                    non-finite cells (any of rho, p, e, U) | lowest label among them (-1: none) | deltaT | time under adjustTimeStep
 *   1 integrals (8): V, rho V, rho Ux V, rho Uy V, rho Uz V, rho E V, rho e V, rho |U|^2/2 V summed over the owned cells
 *   2 extrema (20):  {min, its cell, max, its cell} of rho, p, T = e/Cv, |U|, Mach = |U|/c over the owned cells whose state is
 *                    finite; ties go to the lowest label; NaN and -1 when there is no such cell
 *   3 probes (7 each):  rho, Ux, Uy, Uz, p, T, e of the probe's cell (NaN where the label is -1)
 *   4 patches (9 each): sum |Sf|, the five net fluxes {phiJm, phiJmU + phiP - phiPi (3), phiJmH + phiQ - phiPiU}, sum p_b Sf (3)
 * Cell labels are those of the unsharded mesh, as doubles.  Ghost cells of a shard and the copies behind cyclic halves are never
 * counted, nor are patch faces they own or faces without fields.  The patch fluxes are those of the assembly that produced the
 * state held (the last step's, or qgd_case_update_fluxes'), so that with the integrals of successive samples they close the
 * discrete balance of mass, momentum and total energy to rounding. */
typedef struct qgd_monitor_s* qgd_monitor_t;
#define QGD_MONITOR_SECTIONS 5
#define QGD_MONITOR_SLOTS 4
typedef struct qgd_monitor_spec {
    int32_t nProbes;            /* probeCells: labels of this device's mesh; -1 = not on this rank (a row of NaN) */
    int32_t nPatches;           /* patches: indices of real patches (a halo, empty, cyclic or wedge patch is refused by name) */
    const int32_t* probeCells;
    const int32_t* patches;
} qgd_monitor_spec;
/* After qgd_case_set_fields.  The monitor belongs to its case: qgd_case_free frees the monitors still open first (a later
 * qgd_monitor_free of such a handle does nothing). */
int qgd_monitor_create(qgd_case_t c, const qgd_monitor_spec* spec, qgd_monitor_t* out);
/* offsets of the sections, doubles in a result block, most workgroups of the cell pass (its lanes stride beyond gridCap * 256 cells) */
int qgd_monitor_layout(qgd_monitor_t m, int64_t offsets[QGD_MONITOR_SECTIONS], int64_t* nDoubles, int32_t* gridCap);
/* Stream-ordered on the case's stream, no host wait: the pass, a copy into pinned host memory of slot 0..3, an event. */
int qgd_monitor_sample(qgd_monitor_t m, int32_t slot);
/* Waits for that slot's event only.  time / step: those of the case when the slot was sampled. */
int qgd_monitor_read(qgd_monitor_t m, int32_t slot, double* out, int64_t cap, double* time, int64_t* step);
int qgd_monitor_free(qgd_monitor_t m);

/* The species block of a monitor, for a case that carries species (qgd_case_set_species): the same quantities per species, all nSpecies
 * in the case's species order, the inert one included.  qgd_monitor_enable_species is called once, after qgd_monitor_create and before the
 * monitor's first sample; from then on every qgd_monitor_sample forms the species block too (three more launches whatever nSpecies is; the
 * block travels in the same copy, into the slot's pinned memory behind the flow block, under the same event).  Until it is called a
 * monitor launches and copies exactly what it did before these entries existed, on a case with species too.  The block follows the
 * flow block's rules: nothing is written to the case, no sum depends on anything but the mesh, the specification and nSpecies (two
 * samples of one state are bitwise equal), ghost cells of a shard, the copies behind cyclic halves and patch faces they own are never
 * counted, labels are those of the unsharded mesh.
 *
 * Species block (doubles; qgd_monitor_species_layout gives the offsets of its QGD_MONITOR_SECTIONS sections), S = nSpecies:
 *   0 header (8):      S | inert index | species flux state (0: no species assembly since qgd_case_set_fields, the patch fluxes are NaN;
 *                      1: explicit branch; 2: implicitDiffusion branch) | owned cells with a non-finite Y_i | lowest label among them
 *                      (-1: none) | max |sum_i Y_i - 1| over the owned cells whose Y_i are all finite (NaN: no such cell) | nProbes | nPatches
 *   1 integrals (S):   sum rho Y_i V over the owned cells, rho from the records
 *   2 extrema (4 S):   {min, its cell, max, its cell} of Y_i over the owned cells whose Y_i is finite; ties go to the lowest label; NaN
 *                      and -1 when there is no such cell
 *   3 probes (S each):  Y_i of the probe's cell (NaN where the label is -1)
 *   4 patches (S each): the total over the patch's faces of the net flux of species i out of the domain, as the species' cell update of
 *                      the last step consumed it.  Explicit branch: phiJmY_i - (muf / Sc_i) snGrad(Y_i) |Sf|.  implicitDiffusion: phiJmY_i
 *                      plus YEqn.flux() on the face, -(a_b / Sc_i)(Y_b - Y_P) with a_b = muf |Sf| delta_f and the new Y_i of the owner, on
 *                      the faces of the species' fixedValue patches (zero elsewhere).  The inert species: phiJm minus the transported
 *                      species' fluxes, what Y_inert = 1 - sum implies.  With the integrals of successive samples they close the
 *                      discrete balance of every species to rounding (explicit branch) or to the residuals of the solves (implicit
 *                      branch) while no clip (Y_i.max(0), the inert max(1 - sum, 0)) is active.  The inert row takes phiJm from the
 *                      assembly the flow block reports: after a qgd_case_update_fluxes that followed the step it is that of the new state.
 * QGD_ERR_INVALID, with the reason named: qgd_monitor_enable_species on a case without species or after the monitor's first sample (a
 * second call on an enabled monitor does nothing); qgd_monitor_species_layout / _read before it; a slot out of range or never sampled;
 * cap below the block's doubles.  These three entries were added without a change of QGD_ABI_VERSION (it stays 9: no struct grew, no
 * existing entry changed its meaning); a host that must run against older builds looks the symbols up. */
int qgd_monitor_enable_species(qgd_monitor_t m);
int qgd_monitor_species_layout(qgd_monitor_t m, int64_t offsets[QGD_MONITOR_SECTIONS], int64_t* nDoubles);
/* Waits for the slot's event only (the one qgd_monitor_read waits for). */
int qgd_monitor_species_read(qgd_monitor_t m, int32_t slot, double* out, int64_t cap);

/* ---- run monitor of a QHD case (QHDFoam, SRFQHDFoam; qgd_qhd_monitor.hip) ------ */
/* The same handle and the same rules for a resident QHD case: three launches and one small copy per sample on the device's stream,
 * nothing written that the case reads, none of its launches changed, every sum a fixed tree (two samples of one state are bitwise
 * equal), owned cells only (ghost cells of a shard are never counted, nor are patch faces they own), labels of the unsharded mesh as
 * doubles.  qgd_monitor_layout / _sample / _read / _free serve the handle unchanged; qgd_monitor_enable_species on it is
 * QGD_ERR_INVALID (a QHD case carries no species).  qgd_qhd_case_free frees the monitors still open on the case first (a later
 * qgd_monitor_free of such a handle does nothing).  On a sharded case (qgd_qhd_case_step_sharded, qgd_qhd_case_step_phase) a sample
 * between whole steps reports this shard's owned cells.
 *
 * Result block (doubles; qgd_monitor_layout gives the offsets of its QGD_MONITOR_SECTIONS sections):
 *   0 header (8):     owned cells | flux state | nProbes | nPatches | cells with a non-finite value in any of U, T, p | lowest label
 *                     among them (-1: none) | deltaT | flags: bit 0 rotating, bit 1 T frozen (qgd_qhd_case_set_srf)
 *                     flux state 0: no step since qgd_qhd_case_set_fields -- patch fluxes and the continuity entries are NaN;
 *                     1: explicit branch -- everything is reported; 2: implicitDiffusion -- the face terms hold the explicit part only:
 *                     the volumetric flux and the continuity entries are reported, the four U / T flux columns are NaN
 *   1 integrals (12): V | U_x V, U_y V, U_z V | T V | |U|^2/2 V | p V | B_x V, B_y V, B_z V | sum_c d_c | sum_c |d_c|, summed over the owned
 *                     cells.  B is the body force as the NEXT step's cell update forms it from this state: beta T g, minus 2 omega ^ U on
 *                     a rotating case.  d_c is the signed sum of phi over all faces of cell c (+ where the cell owns the face): entries
 *                     10 and 11 are OpenFOAM's global and local continuity errors before the factor deltaT / sum V
 *   2 extrema (16):   {min, its cell, max, its cell} of |U|, T, p and |d_c| / V_c over the owned cells whose state is finite; ties go to
 *                     the lowest label; NaN and -1 when there is no such cell, and for the continuity row under flux state 0
 *   3 probes (5 each):  Ux, Uy, Uz, T, p of the probe's cell (NaN where the label is -1)
 *   4 patches (9 each): sum |Sf| | sum phi | the totals of the three net face terms of the U equation | that of the T equation (NaN when
 *                     T is frozen) | sum p_b Sf (3).  The face terms are what the cell update of the last step consumed, so that with the
 *                     integrals of successive samples and the body force they close the discrete balances of U and T to rounding.
 * qgd_qhd_case_get_field knows "faceTerms" for the checks of these totals: the four net face terms by face label, 4 nF doubles,
 * component-major; valid after a step (QGD_ERR_INVALID before); under implicitDiffusion the explicit part.
 * This entry and that name were added without a change of QGD_ABI_VERSION (it stays 9: no struct grew, no existing entry changed its
 * meaning); a host that must run against older builds looks the symbol up. */
int qgd_qhd_monitor_create(qgd_qhd_case_t c, const qgd_monitor_spec* spec, qgd_monitor_t* out);

#ifdef __cplusplus
}
#endif
#endif /* QGD_AMD_H */
