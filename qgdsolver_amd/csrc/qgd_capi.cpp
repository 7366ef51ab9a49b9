// qgd_capi.cpp -- the C-ABI of include/qgd_amd.h (compiled with hipcc).
//
// One handle == one HIP device == one calling host thread.  Entries are
// synchronous at return unless documented otherwise.  No exceptions cross the
// boundary: every entry catches and converts to a status code, mirroring how the
// reference turns failures into FatalError exits [fvsc_8C_source.html L62,75-78].
// There is NO CPU fallback: without a HIP device the device/case entries fail
// with QGD_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // declarations only: RCCL is bound at run time (dlopen), the library does not link it

#include <algorithm>
#include <cmath>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <functional>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/qgd_amd.h"
#include "qgd_device.hpp"
#include "qgd_mesh.hpp"
#include "qgd_setup.hpp"

using namespace qgd;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_lastError;
static int fail(int code, const std::string& msg) {
    g_lastError = msg;
    return code;
}
struct HipError : std::runtime_error {
    explicit HipError(const std::string& s) : std::runtime_error(s) {}
};
#define HIP_CHECK(expr)                                                                                     \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            (void)hipGetLastError(); /* reported here, once: a later hipGetLastError() must not see it */   \
            throw HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " at " + __FILE__ + ":" +   \
                           std::to_string(__LINE__));                                                       \
        }                                                                                                   \
    } while (0)
#define QGD_TRY try {
#define QGD_CATCH                                                                 \
    }                                                                             \
    catch (const HipError& e) { return fail(QGD_ERR_HIP, e.what()); }             \
    catch (const std::invalid_argument& e) { return fail(QGD_ERR_INVALID, e.what()); } \
    catch (const std::exception& e) { return fail(QGD_ERR_INVALID, e.what()); }   \
    catch (...) { return fail(QGD_ERR_INVALID, "unknown exception"); }

// ---------------------------------------------------------------------------
// handle types
// ---------------------------------------------------------------------------
struct qgd_mesh_s {
    HostMesh m;
};

struct DeviceArena {
    std::vector<void*> ptrs;
    int64_t bytes = 0;
    void* raw(size_t nbytes) {
        void* d = nullptr;
        HIP_CHECK(hipMalloc(&d, nbytes));
        ptrs.push_back(d);
        bytes += (int64_t)nbytes;
        return d;
    }
    template <class T, class Al>
    T* upload(const std::vector<T, Al>& v) {
        if (v.empty()) return nullptr;
        void* d = raw(v.size() * sizeof(T));
        HIP_CHECK(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return (T*)d;
    }
    template <class T>
    T* alloc(size_t n, bool zero = true) {
        if (n == 0) return nullptr;
        void* d = raw(n * sizeof(T));
        if (zero) { HIP_CHECK(hipMemset(d, 0, n * sizeof(T))); HIP_CHECK(hipStreamSynchronize(nullptr)); }   // see PressureSolver::alloc
        return (T*)d;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
        bytes = 0;
    }
};

// Persistent per-device workspace of the host-pointer operator entries (qgd_fvsc_*, qgd_interpolate, qgd_qhd_*,
// qgd_species_flux): grow-only device buffers by slot, and two pinned staging chunks through which pageable caller memory
// is moved in a double-buffered pipeline (the host copy of chunk k+1 overlaps the DMA of chunk k).  Nothing is allocated
// or freed per call once the sizes have been seen.
struct Workspace {
    struct Buf { void* p = nullptr; size_t cap = 0; };
    std::vector<Buf> dev;
    void* pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    static constexpr size_t CHUNK = (size_t)32 << 20;
    int64_t bytes = 0;

    template <class T>
    T* get(size_t slot, size_t n) {
        if (dev.size() <= slot) dev.resize(slot + 1);
        const size_t need = std::max<size_t>(n, 1) * sizeof(T);
        Buf& b = dev[slot];
        if (b.cap < need) {
            if (b.p) { (void)hipFree(b.p); bytes -= (int64_t)b.cap; b.p = nullptr; b.cap = 0; }
            HIP_CHECK(hipMalloc(&b.p, need));
            b.cap = need; bytes += (int64_t)need;
        }
        return (T*)b.p;
    }
    void ensurePinned() {
        if (pin[0]) return;
        for (int i = 0; i < 2; ++i) {
            HIP_CHECK(hipHostMalloc(&pin[i], CHUNK, hipHostMallocDefault));
            HIP_CHECK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
    }
    static bool devAccessible(const void* p) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
        return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
    }
    static void hostCopy(void* dst, const void* src, size_t n) {
        const int64_t blocks = (int64_t)((n + ((size_t)1 << 20) - 1) >> 20);
#pragma omp parallel for schedule(static) if (blocks > 4)
        for (int64_t b = 0; b < blocks; ++b) {
            const size_t off = (size_t)b << 20;
            std::memcpy((char*)dst + off, (const char*)src + off, std::min<size_t>((size_t)1 << 20, n - off));
        }
    }
    // host -> device, stream-ordered on s; returns when the source may be reused
    void h2d(void* dst, const void* src, size_t n, hipStream_t s) {
        if (!n) return;
        if (devAccessible(src)) { HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, s)); HIP_CHECK(hipStreamSynchronize(s)); return; }
        ensurePinned();
        int k = 0;
        for (size_t off = 0; off < n; off += CHUNK, k ^= 1) {
            const size_t len = std::min(CHUNK, n - off);
            HIP_CHECK(hipEventSynchronize(ev[k]));
            hostCopy(pin[k], (const char*)src + off, len);
            HIP_CHECK(hipMemcpyAsync((char*)dst + off, pin[k], len, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipEventRecord(ev[k], s));
        }
    }
    // device -> host, after everything queued on s; returns when dst holds the data
    void d2h(void* dst, const void* src, size_t n, hipStream_t s) {
        if (!n) return;
        if (devAccessible(dst)) { HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, s)); HIP_CHECK(hipStreamSynchronize(s)); return; }
        ensurePinned();
        HIP_CHECK(hipEventSynchronize(ev[0]));
        HIP_CHECK(hipEventSynchronize(ev[1]));
        size_t prevOff = 0, prevLen = 0;
        int k = 0;
        for (size_t off = 0; off < n; off += CHUNK, k ^= 1) {
            const size_t len = std::min(CHUNK, n - off);
            HIP_CHECK(hipMemcpyAsync(pin[k], (const char*)src + off, len, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipEventRecord(ev[k], s));
            if (prevLen) { HIP_CHECK(hipEventSynchronize(ev[k ^ 1])); hostCopy((char*)dst + prevOff, pin[k ^ 1], prevLen); }
            prevOff = off; prevLen = len;
        }
        HIP_CHECK(hipEventSynchronize(ev[k ^ 1]));
        hostCopy((char*)dst + prevOff, pin[k ^ 1], prevLen);
    }
    void release() {
        for (Buf& b : dev) if (b.p) (void)hipFree(b.p);
        dev.clear();
        for (int i = 0; i < 2; ++i) {
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            pin[i] = nullptr; ev[i] = nullptr;
        }
        bytes = 0;
    }
};

// Who owns which slot of Workspace::dev.  The WORK slots WS_CELL, WS_BND, WS_PT, WS_OUT and WS_H belong to the code that launches on device
// pointers (the *_dev entries, and the host entries that launch themselves: fvsc, interpolate, flux_upwind): records, vertex values and
// outputs in SoA.  A host-pointer entry that runs device-pointer code stages its arguments in slots from WS_STAGE upwards, through a Stager,
// and fetches multi-component results through WS_XPOSE (fetchFaceSoA); no device-pointer code names either, so the two cannot alias.
// WS_A and WS_B are extra arrays of host entries that launch themselves: qgd_flux_upwind (the flux), qgd_scalar_case_get_field (its debug
// block), and qgd_qhd_case_set_fields / qgd_scalar_case_set_fields, which stage the caller's fields in WS_CELL, WS_A and WS_B before their own
// kernels copy them into the case -- they call no device-pointer code, so the work slot they borrow is free.
enum WsSlot { WS_CELL = 0, WS_BND, WS_PT, WS_OUT, WS_H, WS_XPOSE, WS_A, WS_B, WS_STAGE };
// hands out the staging slots of one host-pointer call in order, and uploads
struct Stager {
    Workspace& ws;
    hipStream_t stream;
    size_t next = WS_STAGE;
    double* scratch(size_t n) { return ws.get<double>(next++, n); }
    double* up(const double* src, size_t n) {
        double* dst = scratch(n);
        if (src && n) ws.h2d(dst, src, sizeof(double) * n, stream);
        return dst;
    }
};

// Tuning knobs of the measurement scripts (QGD_*): a value outside the supported set is an error, not a silent change of
// code path.  allowed == nullptr: any integer in [lo, hi].
static int envChoice(const char* name, int dflt, const int* allowed, int nAllowed, int lo = 0, int hi = 0) {
    const char* e = std::getenv(name);
    if (!e || !*e) return dflt;
    char* end = nullptr;
    const long v = std::strtol(e, &end, 10);
    bool ok = end && *end == '\0';
    if (ok && allowed) { ok = false; for (int i = 0; i < nAllowed; ++i) ok = ok || allowed[i] == v; }
    else if (ok) ok = v >= lo && v <= hi;
    if (!ok) throw std::invalid_argument(std::string(name) + "=" + e + " is not a supported value");
    return (int)v;
}
static int envOnOff(const char* name, int dflt) {   // the two-valued knobs
    static const int kOnOff[] = {0, 1};
    return envChoice(name, dflt, kOnOff, 2);
}
static double nowMs() {
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e3 * (double)t.tv_sec + 1e-6 * (double)t.tv_nsec;
}

// ---- constraint patches in the resident cases -----------------------------------------------------------------------------------------
// OpenFOAM gives a field on a constraint patch the patch's own field type whatever the field file says (L0: fvPatchField<Type>::New,
// "patchFieldType overridden by the patch's constraint type"): empty patches and the cut planes of a shard carry nothing;
// symmetryPlane / symmetry reflect vectors (symmetryPlaneFvPatchField / basicSymmetryFvPatchField: evaluate = (pif +
// transform(I - 2 nn, pif))/2) and leave scalars zero-gradient.  The stencils know the same list
// [extendedFaceStencilScalarGrad.C L90-101, GaussVolPointBase3D.C L783-794].
static void constraintKinds(int ptype, int32_t& bcU, int32_t& bcT, int32_t& bcP) {
    if (ptype == QGD_PATCH_EMPTY || ptype == QGD_PATCH_HALO) { bcU = bcT = bcP = QGD_BC_NONE; }
    else if (ptype == QGD_PATCH_SYMMETRYPLANE || ptype == QGD_PATCH_SYMMETRY) { bcU = QGD_BC_SLIP; bcT = bcP = QGD_BC_ZEROGRADIENT; }
}
static void initPatchBC(PatchBCDev& b, const Patch& p) {
    std::memset(&b, 0, sizeof(b));
    b.ptype = p.type;
    b.bcU = b.bcT = b.bcP = QGD_BC_ZEROGRADIENT;
    constraintKinds(p.type, b.bcU, b.bcT, b.bcP);
    if (p.type == QGD_PATCH_SYMMETRYPLANE && (p.size > 0 || p.nHatInherited)) {
        b.planeN = 1;
        for (int k = 0; k < 3; ++k) b.nHat[k] = p.nHat[k];
    }
}
static void residentCasePatchCheck(const HostMesh& m, std::string& why, int& code) {
    why.clear(); code = 0;
    for (const Patch& p : m.patches) {
        if ((p.type == QGD_PATCH_CYCLIC || p.type == QGD_PATCH_WEDGE) && p.nonEmptyGlobally()) {
            why = std::string("patch '") + p.name + "' is a " + (p.type == QGD_PATCH_CYCLIC ? "cyclic" : "wedge") +
                  " patch: the resident cases do not serve coupled / wedge patch fields (use the fvsc operators, which do)";
            code = QGD_ERR_NOT_IMPLEMENTED;
            return;
        }
        if (p.type == QGD_PATCH_SYMMETRYPLANE) {
            for (int32_t f = p.start; f < p.start + p.size; ++f) {   // L0: symmetryPlanePolyPatch::calcGeometry, magSqr(n_ - nf) > SMALL is fatal
                double d2 = 0;
                for (int k = 0; k < 3; ++k) { const double x = p.nHat[k] - m.Sf[3 * (size_t)f + k] / m.magSf[f]; d2 += x * x; }
                if (d2 > 1e-15) { why = std::string("Symmetry plane '") + p.name + "' is not planar (use the symmetry patch type)"; code = QGD_ERR_INVALID; return; }
            }
        }
    }
}

struct qgd_device_s {
    int deviceId = 0;
    Workspace ws;
    double opMs[3] = {0, 0, 0};  // last host-pointer operator call: host->device, kernels, device->host (qgd_device_op_times)
    hipEvent_t opEv[2] = {nullptr, nullptr};
    DeviceArena arena;
    MeshView view{};
    int32_t nGeomD = 3;
    bool hasTri = false;
    bool wedgePrism = false;  // wedge patches + prism cells: GaussVolPoint is refused [fvsc_8C L65-82]
    int64_t fusedInfo[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // qgd_device_fused_blocks
    int64_t fusedFacesComputed = 0;   // internal faces the fused kernel's blocks compute per step, surface faces once per side (MeshView::fuBlocks > 0)
    int64_t fusedCellsStaged = 0, fusedCellsStagedFull = 0, fusedVertsStaged = 0;   // cell records / of which with RecB and centre / vertices its blocks stage per step
    std::vector<Patch> patches;
    // why a resident case (qgd_case_create / qgd_qhd_case_create) cannot run on this mesh, empty when it can: cyclic / wedge patches
    // with faces (their coupled / rotated patch fields are not served), a symmetryPlane that is not planar (fatal in OpenFOAM too)
    std::string caseRefusal; int caseRefusalCode = 0;
    std::vector<double> hf;  // host copy of hQGDf for the accessor
    // varScModel7 (VarScView::rf): r_f per face, -1 on faces without fields; the device copy is made when the first case asks for the model
    std::vector<double> sensorRatio;
    const double* sensorRatioDev = nullptr;
    const double* ensureSensorRatio() {
        if (!sensorRatioDev && !sensorRatio.empty()) sensorRatioDev = arena.upload(sensorRatio);
        return sensorRatioDev;
    }
    // halo lists (device) and sizes, one entry per halo slot (neighbouring shard)
    struct HaloSlot {
        int32_t *ghost = nullptr, *send = nullptr, *ghostBF = nullptr, *sendBF = nullptr;
        int32_t nGhost = 0, nSend = 0, nGhostBF = 0, nSendBF = 0;
    };
    std::vector<HaloSlot> halo;
    // cyclic patch pairs served by ghost cells (qgd_mesh_unroll_cyclic): slot k unpacks what slot haloSelf[k] of the SAME case packs
    std::vector<int32_t> haloSelf;
    bool periodic() const { if (haloSelf.empty()) return false; for (int32_t x : haloSelf) if (x < 0) return false; return true; }
    bool sharded() const { for (const HaloSlot& h : halo) if (h.nGhost || h.nSend) return true; return false; }
    int32_t ownedBegin = 0, ownedEnd = 0;      // local labels of the owned cells (contiguous by construction of the shard builders)
    std::vector<int32_t> cellGlobal;           // extracted shards: label in the unsharded mesh per local cell (ascending)
    int64_t cellGlobalOffset = 0;              // box slabs: global label = local label + offset
    // local label of a cell of the unsharded mesh, -1 when this shard does not OWN it
    int32_t ownedLocalOf(int64_t globalCell) const {
        int64_t local = -1;
        if (!cellGlobal.empty()) {
            auto it = std::lower_bound(cellGlobal.begin(), cellGlobal.end(), (int32_t)globalCell);
            if (it != cellGlobal.end() && *it == globalCell) local = it - cellGlobal.begin();
        } else local = globalCell - cellGlobalOffset;
        return (local >= ownedBegin && local < ownedEnd) ? (int32_t)local : -1;
    }
    int32_t* sendAll = nullptr;     // send cells of every slot (each cell once)
    int32_t* sendBFAll = nullptr;   // their real-patch boundary faces
    int32_t nSendAll = 0, nSendBFAll = 0;
    hipStream_t stream = nullptr;
    int liveCases = 0;   // qgd_case_t / qgd_qhd_case_t created on this device and not freed yet (qgd_device_free refuses while > 0)
    ImplicitSolver* opSolver = nullptr;   // the linear solver of the stateless implicit operators (qgd_species_step_implicit), made on first use
    // MeshView::geoPos, built the first time a case that takes fvc::grad(U) per cell is created on this device (QGD_GEOPOS=0: never)
    void ensureFaceGeoPos() {
        if (view.geoPos || view.nF == 0 || !envOnOff("QGD_GEOPOS", 1)) return;
        double4* g = arena.alloc<double4>((size_t)view.nF, false);
        (void)hipGetLastError();   // a stale error of an earlier, refused call must not be taken for this launch's
        launchFaceGeoPos(stream, view, g);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(stream));
        view.geoPos = g;
    }
};

struct TimedLaunch {
    int k;
    hipEvent_t a, b;
};

// One halo message of a case (QGD case: kind 0 state, 1 grad U, 2 U, 3 search direction, 4 guess, 5 mid-assembly; QHD case: kinds 0..4,
// include/qgd_amd.h): its length per cell / per patch face of a slot's lists, and the launch that packs it into, or unpacks it from, a buffer
struct HaloMessage {
    int perCell = 0, perFace = 0;
    std::function<int(int slot, double* buf, bool pack, hipStream_t stream)> move;   // QGD_OK, or what fail() returned
    size_t sendCount(const qgd_device_s::HaloSlot& h) const { return (size_t)perCell * h.nSend + (size_t)perFace * h.nSendBF; }
    size_t recvCount(const qgd_device_s::HaloSlot& h) const { return (size_t)perCell * h.nGhost + (size_t)perFace * h.nGhostBF; }
};
// The message buffers of a case's own transport (exchangeOn), per halo slot, sized on first use for the widest message of the case.
// ONE pair serves every message kind, the cyclic self-exchange included, because no two exchanges of a case are ever in flight together:
// all of them are enqueued on the case's stream, in program order, except the state exchange of the overlapped step
// (qgd_case_step_sharded), which runs on the library's halo stream -- and there the compute stream waits on evUnpacked, the event
// behind that exchange's last unpack, before the step returns, so whatever could issue the next message (the next step's
// mid-assembly exchange at the earliest) is ordered after the buffers' last use.  (qgd_case_set_stream waits for the old stream first.)
struct HaloBuffers {
    DeviceArena* arena = nullptr;
    HaloMessage widest;   // its widths only
    std::vector<double*> send, recv;
    void ensure(const qgd_device_s* d) {
        if (send.size() == d->halo.size()) return;
        send.assign(d->halo.size(), nullptr);
        recv.assign(d->halo.size(), nullptr);
        for (size_t s = 0; s < d->halo.size(); ++s) {
            send[s] = arena->alloc<double>(widest.sendCount(d->halo[s]));
            recv[s] = arena->alloc<double>(widest.recvCount(d->halo[s]));
        }
    }
};

// What the three resident cases (qgd_case_s, qgd_qhd_case_s, qgd_scalar_case_s) share, and what the entries that work on these members
// alone take: the patch table, the per-face value lists, the implicit solve's accessors, the stream wait, the public halo entries, the
// monitors and the teardown.  A plain base: the handles stay the three structs, which add their own members.
struct qgd_monitor_s;
struct CaseCore {
    qgd_device_s* dev = nullptr;
    int stencil = ST_GVP3;      // device stencil kind
    bool usesPoints = true;
    bool fieldsSet = false;
    bool counted = false;       // dev->liveCases counts this case (the last thing a create does)
    std::vector<PatchBCDev> bc;
    PatchBCDev* bcDev = nullptr;
    DeviceArena arena;
    double time = 0;
    int64_t steps = 0;
    // the implicitDiffusion branch's linear solver (device-scalar multi-right-hand-side): the U and e solves of a QGD case, the four systems
    // {Ux, Uy, Uz, T} of a QHD case as one solve, the T equation of a scalar case; nullptr without the branch
    ImplicitSolver* implSolver = nullptr;
    HaloBuffers haloBuf;        // native halo transport (exchangeOn): the message buffers
    std::vector<qgd_monitor_s*> monitors;   // qgd_monitor_create / qgd_qhd_monitor_create: freed with the case where still open
    // optional caller-owned stream (e.g. the one RCCL transfers are ordered on): qgd_case_set_stream, a QGD case only
    hipStream_t userStream = nullptr;
    bool useUserStream = false;
    hipStream_t stream() const { return useUserStream ? userStream : dev->stream; }
};

// the handle of a run monitor (its entries: "run monitors" below); here because a case frees the monitors still open on it
struct qgd_monitor_s {
    CaseCore* c = nullptr;
    bool qhd = false;            // the kind of the handle: c is a qgd_qhd_case_s (qgd_qhd_monitor_create), else a qgd_case_s
    MonitorView view{};
    DeviceArena arena;
    double* result = nullptr;    // device: one result block (the copy into a slot follows the fold in stream order)
    double* host = nullptr;      // pinned: QGD_MONITOR_SLOTS slots of nDoubles + spDoubles: the flow block, the species block behind it
    int64_t nDoubles = 0;
    // the species block (qgd_monitor_enable_species; qgd_monitor_species.hip): spDoubles == 0 until it is enabled
    SpeciesMonitorView spView{};
    int64_t spDoubles = 0;
    hipEvent_t ev[QGD_MONITOR_SLOTS] = {};
    bool sampled[QGD_MONITOR_SLOTS] = {};
    double time[QGD_MONITOR_SLOTS] = {};
    int64_t step[QGD_MONITOR_SLOTS] = {};
};
// the open monitors of this process: a handle whose case was freed first is no longer among them
static std::vector<qgd_monitor_s*> g_monitors;
static bool monitorLive(const qgd_monitor_s* m) { return m && std::find(g_monitors.begin(), g_monitors.end(), m) != g_monitors.end(); }
static void monitorDestroy(qgd_monitor_s* m) {
    for (hipEvent_t e : m->ev) if (e) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
    if (m->host) (void)hipHostFree(m->host);
    m->arena.release();
    g_monitors.erase(std::remove(g_monitors.begin(), g_monitors.end(), m), g_monitors.end());
    delete m;
}
// The one teardown of a case's core, from the catch of a create and from a free alike, after the kind's own extras (pressure solver, timing
// events, own halo stream): the monitors still open and the solver once the stream has drained, the arena, the device's count.  The caller
// deletes the handle.
static void caseTeardown(CaseCore* c) {
    if (!c->monitors.empty() || c->implSolver) (void)hipStreamSynchronize(c->stream());
    for (qgd_monitor_s* m : c->monitors) monitorDestroy(m);
    c->monitors.clear();
    if (c->implSolver) implicitSolverFree(c->implSolver);
    c->arena.release();
    if (c->counted) c->dev->liveCases--;
}
// every exit of a create after `new` that does not hand the case out
template <class Case>
static int caseAbandon(Case* c, int rc) {
    caseTeardown(c);
    delete c;
    return rc;
}

struct qgd_case_s : CaseCore {
    qgd_case_options opt{};
    GasModel gas{};
    // per-term fvsc entries (qgd_case_options::termStencil): mixB >= 0: the case walks its faces with the two stencils stencil < mixB, the
    // gradient components in mixMask by mixB (bit k: rho, Ux, Uy, Uz, p, e)
    int mixB = -1, mixMask = 0;
    int implXOrder = 0;         // QGD_IMPL_XEXTRAP: order of the start-value extrapolation of the implicit branch's solves (ImplView::have counts up to it)
    bool pRefresh = true;       // grad(p)'s word is GaussVolPoint: p's boundary conditions are re-evaluated inside it [GaussVolPointStencil_8C L73] (quirk B6)
    bool fused = false;         // qgd_case_step advances with fusedFaceCellKernel (QGD_FUSED)
    bool fusedAdj = false;      // adjustTimeStep: the blocks run up to their flux sums + Courant partials, cellFinishKernel advances once deltaT is known (QGD_FUSED_ADJUST)
    bool fusedImpl = false;     // implicitDiffusion: vertex values, QGD fluxes, tauMC and the U systems' rows are one launch on the same blocks (QGD_IMPL_FUSED)
    bool ghostsCurrent = false;     // cyclic pairs served by ghost cells (selfHaloExchange): whether the copies hold their originals' records: reset by set_fields (the only way on after set_bc / set_qgd_coeffs, which
                                    //     clear fieldsSet), set by qgd_case_step and qgd_case_update_fluxes, which refresh the copies first; qgd_case_step_phase is refused
    bool hasQgdFlux = false;
    bool phiwRegistered = false;
    bool fluxAssembled = false;     // CaseView::flux holds the fluxes of an assembly of this case's fields (what a monitor reports per patch)
    // per-face values of fixedValue patches (qgd_case_set_bc_values), field 0 U (3 per boundary face), 1 T, 2 p: the host copy serves
    // qgd_case_get_bc_values, the device copy is CaseView::bValU / bValT / bValP while some patch's valList names the field; both empty /
    // nullptr until the first list arrives
    std::vector<double> bcValHost[3];
    double* bcValDev[3] = {nullptr, nullptr, nullptr};
    CaseView view{};
    double* dbgBuf = nullptr;
    ImplView impl{};            // implicitDiffusion branch: its face / cell work arrays (CaseCore::implSolver runs its two linear solves)
    int implSolveIndex = 0;                 // 0: the U solve is the one in flight, 1: the e solve
    bool reuseGradU = true;                 // QGD_IMPL_REUSE_GRADU (default 1)
    bool gradUValid = false;                // implicit branch, unsharded: fvc::grad(U) of phase 29 is still that of the records (phase 20 of the next step skips it)
    double* coef[4] = {nullptr, nullptr, nullptr, nullptr};  // device copies of non-uniform alphaQGD / ScQGD (cells, patch faces)
    // varScModel7 (qgd_case_set_var_sc): the sensor writes coef[2], which CaseView::sc reads; coef[3] holds the clipped dictionary value
    bool varSc = false;
    VarScView vsc{};
    uint8_t* constCellDev = nullptr;
    double* scPart = nullptr;   // partials of qgd_case_sc_range
    // species mass fractions (qgd_case_set_species; qgd_species.hip): sp.nS == 0: none.  The host tables of the per-species per-patch boundary
    // conditions go to the device, and the patch values are evaluated from them, before the first use after a change (spDirty)
    SpeciesView sp{};
    std::vector<uint8_t> spBcKind, spFieldSet;
    std::vector<double> spBcVal;
    uint8_t* spBcKindDev = nullptr;
    double* spBcValDev = nullptr;
    bool spDirty = false, spKeep = false, spFluxesValid = false;
    bool spHalo = false;        // QGD_SPECIES_HALO: the state message (kind 0) carries the composition behind the flow's records
    // the implicitDiffusion branch of the species [QGDYEqn.H L47-66]: rows and solutions, the statistics of the batches' solves, the controls
    // of qgd_case_set_species_solver (< 0: the case's implicitTol / implicitMaxIter)
    SpeciesImplView spImpl{};
    double* spStats = nullptr;
    int spBatches = 0;
    double spTol = -1.0;
    int32_t spMaxIter = -1;
    // timing
    bool timing = false;
    std::vector<TimedLaunch> pending;
    std::vector<hipEvent_t> freeEvents;
    double totalMs[QGD_K_COUNT] = {};
    int64_t launches[QGD_K_COUNT] = {};
    hipEvent_t curStart = nullptr;
    hipStream_t haloStream = nullptr;  // pack/unpack stream (defaults to stream())
    bool useHaloStream = false;
    // native halo transport (qgd_case_halo_exchange, qgd_case_step_sharded, selfHaloExchange): CaseCore::haloBuf, and the events ordering the two streams
    hipStream_t ownHaloStream = nullptr;
    hipEvent_t evLayerDone = nullptr, evUnpacked = nullptr;
};

static hipEvent_t getEvent(qgd_case_s* c) {
    if (!c->freeEvents.empty()) {
        hipEvent_t e = c->freeEvents.back();
        c->freeEvents.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
static void timingPre(void* ctx, int) {
    qgd_case_s* c = (qgd_case_s*)ctx;
    if (!c->timing) return;
    c->curStart = getEvent(c);
    if (c->curStart) (void)hipEventRecord(c->curStart, c->stream());
}
static void timingPost(void* ctx, int k) {
    qgd_case_s* c = (qgd_case_s*)ctx;
    if (!c->timing || !c->curStart) return;
    hipEvent_t e = getEvent(c);
    if (!e) return;
    (void)hipEventRecord(e, c->stream());
    c->pending.push_back(TimedLaunch{k, c->curStart, e});
    c->curStart = nullptr;
}
static void harvestTiming(qgd_case_s* c) {
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream());
    for (TimedLaunch& t : c->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            c->totalMs[t.k] += ms;
            c->launches[t.k]++;
        }
        c->freeEvents.push_back(t.a);
        c->freeEvents.push_back(t.b);
    }
    c->pending.clear();
}
static Launcher launcherOf(qgd_case_s* c) {
    Launcher L;
    L.stream = c->stream();
    L.pre = timingPre;
    L.post = timingPost;
    L.ctx = c;
    return L;
}

// The OpenMP runtime hipcc links spin-waits between parallel regions by default;
// on oversubscribed hosts that makes the (short) setup loops slower than serial.
__attribute__((constructor)) static void qgdInitOpenMP() { setenv("KMP_BLOCKTIME", "0", 0); }

// ---------------------------------------------------------------------------
extern "C" {

const char* qgd_version(void) { return "qgdsolver_amd 0.1 (gfx950)"; }
const char* qgd_last_error(void) { return g_lastError.c_str(); }
int qgd_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- mesh -----------------------------------------------------------------------
int qgd_mesh_create(int32_t nPoints, const double* points, int32_t nFaces, const int32_t* faceOffsets, const int32_t* facePoints,
                    int32_t nInternalFaces, const int32_t* owner, const int32_t* neighbour, int32_t nCells, int32_t nPatches,
                    const int32_t* patchStart, const int32_t* patchSize, const int32_t* patchType, qgd_mesh_t* out) {
    QGD_TRY
    if (!points || !faceOffsets || !facePoints || !owner || (!neighbour && nInternalFaces > 0) || !out)
        return fail(QGD_ERR_INVALID, "qgd_mesh_create: null argument");
    if (nPoints <= 0 || nFaces <= 0 || nCells <= 0 || nInternalFaces < 0 || nInternalFaces > nFaces || nPatches < 0)
        return fail(QGD_ERR_INVALID, "qgd_mesh_create: bad sizes");
    qgd_mesh_s* h = new qgd_mesh_s();
    HostMesh& m = h->m;
    m.nPoints = nPoints; m.nFaces = nFaces; m.nInternalFaces = nInternalFaces; m.nCells = nCells;
    m.points.assign(points, points + 3 * (size_t)nPoints);
    m.faceOffsets.assign(faceOffsets, faceOffsets + nFaces + 1);
    m.facePoints.assign(facePoints, facePoints + faceOffsets[nFaces]);
    m.owner.assign(owner, owner + nFaces);
    if (nInternalFaces) m.neighbour.assign(neighbour, neighbour + nInternalFaces);
    for (int i = 0; i < nPatches; ++i) {
        Patch p;
        p.name = "patch" + std::to_string(i);
        p.type = patchType[i]; p.start = patchStart[i]; p.size = patchSize[i];
        m.patches.push_back(p);
    }
    std::string err = m.check();
    if (!err.empty()) { delete h; return fail(QGD_ERR_INVALID, "qgd_mesh_create: " + err); }
    m.computeGeometry();
    *out = h;
    return QGD_OK;
    QGD_CATCH
}

int qgd_mesh_box(int32_t nx, int32_t ny, int32_t nzGlobal, int32_t kLo, int32_t kHi, const double lo[3], const double hi[3],
                 const int32_t patchTypes[6], qgd_mesh_t* out) {
    QGD_TRY
    if (!lo || !hi || !out) return fail(QGD_ERR_INVALID, "qgd_mesh_box: null argument");
    qgd_mesh_s* h = new qgd_mesh_s();
    try { h->m = makeBox(nx, ny, nzGlobal, kLo, kHi, lo, hi, patchTypes); }
    catch (...) { delete h; throw; }
    *out = h;
    return QGD_OK;
    QGD_CATCH
}

int qgd_mesh_forward_step(int32_t nx, int32_t ny, int32_t ixStep, int32_t iyStep, double lx, double ly, double lz, qgd_mesh_t* out) {
    QGD_TRY
    if (!out) return fail(QGD_ERR_INVALID, "qgd_mesh_forward_step: null argument");
    qgd_mesh_s* h = new qgd_mesh_s();
    try { h->m = makeForwardStep(nx, ny, ixStep, iyStep, lx, ly, lz); }
    catch (...) { delete h; throw; }
    *out = h;
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_jitter(qgd_mesh_t m, double amplitude, uint64_t seed) {
    QGD_TRY
    if (!m) return fail(QGD_ERR_INVALID, "null mesh");
    jitterPoints(m->m, amplitude, seed);
    m->m.haloFaceH.clear();   // the cut faces' hQGDf of the unsharded mesh no longer describes these points: back to the local rule
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_split_quads(qgd_mesh_t m, int32_t stride) {
    QGD_TRY
    if (!m) return fail(QGD_ERR_INVALID, "null mesh");
    splitQuads(m->m, stride);
    m->m.haloFaceH.clear();   // face lists changed: the per-halo-face values would be misaligned
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_split_edges(qgd_mesh_t m, int32_t stride) {
    QGD_TRY
    if (!m) return fail(QGD_ERR_INVALID, "null mesh");
    splitEdges(m->m, stride);
    m->m.haloFaceH.clear();
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_set_geometry(qgd_mesh_t mh, const double* Sf, const double* Cf, const double* C, const double* V) {
    QGD_TRY
    if (!mh || !Sf || !Cf || !C || !V) return fail(QGD_ERR_INVALID, "qgd_mesh_set_geometry: null argument");
    HostMesh& m = mh->m;
    m.Sf.assign(Sf, Sf + 3 * (size_t)m.nFaces);
    m.Cf.assign(Cf, Cf + 3 * (size_t)m.nFaces);
    m.C.assign(C, C + 3 * (size_t)m.nCells);
    m.V.assign(V, V + (size_t)m.nCells);
    for (int32_t f = 0; f < m.nFaces; ++f) {
        const double* S = &m.Sf[3 * (size_t)f];
        m.magSf[f] = std::sqrt(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]);
    }
    m.userGeometry = true;
    m.haloFaceH.clear();      // computed from the library's own centres; the caller's geometry rules now
    m.computeDerived();
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_set_degenerate_faces(qgd_mesh_t mh, int32_t n, const int32_t* faces) {
    QGD_TRY
    if (!mh || n < 0 || (n > 0 && !faces)) return fail(QGD_ERR_INVALID, "qgd_mesh_set_degenerate_faces: bad argument");
    HostMesh& m = mh->m;
    for (int32_t i = 0; i < n; ++i)
        if (faces[i] < 0 || faces[i] >= m.nFaces) return fail(QGD_ERR_INVALID, "qgd_mesh_set_degenerate_faces: face label out of range");
    m.degenerateFaces.assign(faces, faces + n);
    std::sort(m.degenerateFaces.begin(), m.degenerateFaces.end());
    m.degenerateFaces.erase(std::unique(m.degenerateFaces.begin(), m.degenerateFaces.end()), m.degenerateFaces.end());
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_free(qgd_mesh_t m) {
    delete m;
    return QGD_OK;
}
int qgd_mesh_sizes(qgd_mesh_t mh, int64_t sizes[7]) {
    if (!mh || !sizes) return fail(QGD_ERR_INVALID, "null argument");
    const HostMesh& m = mh->m;
    sizes[0] = m.nPoints; sizes[1] = m.nFaces; sizes[2] = m.nInternalFaces; sizes[3] = m.nCells;
    sizes[4] = (int64_t)m.patches.size(); sizes[5] = (int64_t)m.facePoints.size(); sizes[6] = m.nGeometricD;
    return QGD_OK;
}
// outBytes < 0: size query, *(int64_t*)out receives the array's size in bytes
int qgd_mesh_get(qgd_mesh_t mh, const char* name, void* out, int64_t outBytes) {
    QGD_TRY
    if (!mh || !name || !out) return fail(QGD_ERR_INVALID, "null argument");
    const HostMesh& m = mh->m;
    const std::string s(name);
    const void* src = nullptr;
    size_t bytes = 0;
    std::vector<int32_t> tmp;
    auto D = [&](const auto& v) { src = v.data(); bytes = v.size() * sizeof(double); };
    auto I = [&](const std::vector<int32_t>& v) { src = v.data(); bytes = v.size() * sizeof(int32_t); };
    if (s == "points") D(m.points);
    else if (s == "faceOffsets") I(m.faceOffsets);
    else if (s == "facePoints") I(m.facePoints);
    else if (s == "owner") I(m.owner);
    else if (s == "neighbour") I(m.neighbour);
    else if (s == "patchStart" || s == "patchSize" || s == "patchType") {
        for (const Patch& p : m.patches) tmp.push_back(s == "patchStart" ? p.start : (s == "patchSize" ? p.size : p.type));
        I(tmp);
    } else if (s.rfind("haloGhost", 0) == 0 || s.rfind("haloSend", 0) == 0) {
        const bool ghost = s[4] == 'G';
        const int slot = std::atoi(s.c_str() + (ghost ? 9 : 8));
        const auto& lists = ghost ? m.haloGhost : m.haloSend;
        if (slot >= 0 && slot < (int)lists.size()) I(lists[slot]); else I(tmp);
    } else if (s == "haloPeer") I(m.haloPeer);
    else if (s == "haloSelf") I(m.haloSelf);
    else if (s == "cellGlobal") I(m.cellGlobal);
    else if (s == "faceGlobal") I(m.faceGlobal);
    else if (s == "pointGlobal") I(m.pointGlobal);
    else if (s == "haloFaceH") D(m.haloFaceH);
    else if (s == "degenerateFaces") I(m.degenerateFaces);
    else if (s == "Sf") D(m.Sf);
    else if (s == "magSf") D(m.magSf);
    else if (s == "Cf") D(m.Cf);
    else if (s == "C") D(m.C);
    else if (s == "V") D(m.V);
    else if (s == "weights") D(m.weights);
    else if (s == "deltaCoeffs") D(m.deltaCoeffs);
    else if (s == "nonOrthDeltaCoeffs") D(m.nonOrthDeltaCoeffs);
    else return fail(QGD_ERR_UNKNOWN_NAME, "qgd_mesh_get: unknown array " + s);
    if (outBytes < 0) { *static_cast<int64_t*>(out) = (int64_t)bytes; return QGD_OK; }
    if ((int64_t)bytes > outBytes) return fail(QGD_ERR_INVALID, "qgd_mesh_get: output too small for " + s);
    if (bytes) std::memcpy(out, src, bytes);
    return QGD_OK;
    QGD_CATCH
}

int qgd_mesh_renumber(qgd_mesh_t mh, const int32_t* newOfOld, int32_t* faceNewOfOld) {
    QGD_TRY
    if (!mh || !newOfOld) return fail(QGD_ERR_INVALID, "qgd_mesh_renumber: null argument");
    if (!mh->m.haloGhost.empty()) return fail(QGD_ERR_INVALID, "qgd_mesh_renumber: renumber before sharding");
    renumberCells(mh->m, newOfOld, faceNewOfOld);
    const std::string err = mh->m.check();
    if (!err.empty()) return fail(QGD_ERR_INVALID, "qgd_mesh_renumber: " + err);
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_rcm_order(qgd_mesh_t mh, int32_t* newOfOld) {
    QGD_TRY
    if (!mh || !newOfOld) return fail(QGD_ERR_INVALID, "qgd_mesh_rcm_order: null argument");
    const std::vector<int32_t> order = cuthillMcKee(mh->m);
    std::memcpy(newOfOld, order.data(), sizeof(int32_t) * order.size());
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_morton_order(qgd_mesh_t mh, int32_t* newOfOld) {
    QGD_TRY
    if (!mh || !newOfOld) return fail(QGD_ERR_INVALID, "qgd_mesh_morton_order: null argument");
    const std::vector<int32_t> order = mortonOrder(mh->m);
    std::memcpy(newOfOld, order.data(), sizeof(int32_t) * order.size());
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_shard(qgd_mesh_t global, int32_t nRanks, const int32_t* cellStart, int32_t rank, qgd_mesh_t* out) {
    QGD_TRY
    if (!global || !cellStart || !out) return fail(QGD_ERR_INVALID, "qgd_mesh_shard: null argument");
    if (nRanks < 1 || rank < 0 || rank >= nRanks) return fail(QGD_ERR_INVALID, "qgd_mesh_shard: rank out of range");
    if (!global->m.haloGhost.empty()) return fail(QGD_ERR_INVALID, "qgd_mesh_shard: the mesh is already a shard");
    if (cellStart[0] != 0 || cellStart[nRanks] != global->m.nCells) return fail(QGD_ERR_INVALID, "qgd_mesh_shard: cellStart must run from 0 to nCells");
    for (int r = 0; r < nRanks; ++r)
        if (cellStart[r + 1] <= cellStart[r]) return fail(QGD_ERR_INVALID, "qgd_mesh_shard: every rank needs at least one cell");
    qgd_mesh_s* h = new qgd_mesh_s();
    try {
        h->m = extractShard(global->m, nRanks, cellStart, rank);
        const std::string err = h->m.check();
        if (!err.empty()) { delete h; return fail(QGD_ERR_INVALID, "qgd_mesh_shard: " + err); }
    } catch (...) { delete h; throw; }
    *out = h;
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_unroll_cyclic(qgd_mesh_t mesh, int32_t nPairs, const int32_t* pairs, qgd_mesh_t* out) {
    QGD_TRY
    if (!mesh || !out || (nPairs > 0 && !pairs)) return fail(QGD_ERR_INVALID, "qgd_mesh_unroll_cyclic: null argument");
    std::vector<std::pair<int32_t, int32_t>> pr;
    if (nPairs > 0) for (int32_t k = 0; k < nPairs; ++k) pr.push_back({pairs[2 * k], pairs[2 * k + 1]});
    else {   // consecutive cyclic patches with faces are the two halves of a pair (how blockMesh / createPatch write them)
        std::vector<int32_t> cyc;
        for (size_t i = 0; i < mesh->m.patches.size(); ++i) if (mesh->m.patches[i].type == QGD_PATCH_CYCLIC && mesh->m.patches[i].size > 0) cyc.push_back((int32_t)i);
        if (cyc.empty() || cyc.size() % 2) return fail(QGD_ERR_INVALID, "qgd_mesh_unroll_cyclic: the mesh has no cyclic patches, or an odd number of them");
        for (size_t i = 0; i < cyc.size(); i += 2) pr.push_back({cyc[i], cyc[i + 1]});
    }
    qgd_mesh_s* h = new qgd_mesh_s();
    try {
        h->m = unrollCyclic(mesh->m, pr);
        const std::string err = h->m.check();
        if (!err.empty()) { delete h; return fail(QGD_ERR_INVALID, "qgd_mesh_unroll_cyclic: " + err); }
    } catch (const std::invalid_argument& e) { delete h; return fail(QGD_ERR_NOT_IMPLEMENTED, e.what()); }
    catch (...) { delete h; throw; }
    *out = h;
    return QGD_OK;
    QGD_CATCH
}
int qgd_mesh_halo_slots(qgd_mesh_t mh, int32_t* nSlots) {
    if (!mh || !nSlots) return fail(QGD_ERR_INVALID, "null argument");
    *nSlots = (int32_t)mh->m.haloGhost.size();
    return QGD_OK;
}

// ---- device ----------------------------------------------------------------------
// prismMatcher + findIndices("wedge") of fvscOpName [fvsc_8C L65-82]: a wedge patch and at least one prism cell
// (five faces: two triangles and three quadrilaterals, six vertices)
static bool hasWedgeAndPrism(const HostMesh& m) {
    bool wedge = false;
    for (const Patch& p : m.patches) wedge = wedge || (p.type == QGD_PATCH_WEDGE && p.size > 0);
    if (!wedge) return false;
    std::vector<uint8_t> nTri((size_t)m.nCells, 0), nQuad((size_t)m.nCells, 0), nOther((size_t)m.nCells, 0);
    auto count = [&](int32_t c, int n) { if (n == 3) nTri[c]++; else if (n == 4) nQuad[c]++; else nOther[c]++; };
    for (int32_t f = 0; f < m.nFaces; ++f) {
        count(m.owner[f], m.faceSize(f));
        if (f < m.nInternalFaces) count(m.neighbour[f], m.faceSize(f));
    }
    for (int32_t c = 0; c < m.nCells; ++c)
        if (nTri[c] == 2 && nQuad[c] == 3 && nOther[c] == 0) return true;
    return false;
}
// fusedChoice: -1 = QGD_FUSED of the environment (default 1), 0 = no block tables, 2 = blocks of any size
static int deviceCreate(qgd_mesh_t mh, int deviceId, int fusedChoice, qgd_device_t* out) {
    QGD_TRY
    if (!mh || !out) return fail(QGD_ERR_INVALID, "qgd_device_create: null argument");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(QGD_ERR_NO_DEVICE, "qgd_device_create: no HIP device (this library has no CPU fallback)");
    if (deviceId < 0 || deviceId >= n) return fail(QGD_ERR_INVALID, "qgd_device_create: bad device id");
    HIP_CHECK(hipSetDevice(deviceId));
    const HostMesh& m = mh->m;
    if (m.patches.size() > QGD_MAX_PATCHES) return fail(QGD_ERR_INVALID, "too many patches");
    // QGD_SETUP_TIMING=1: where the device's set-up time goes, stage by stage, on stderr
    const bool stageTiming = std::getenv("QGD_SETUP_TIMING") && std::atoi(std::getenv("QGD_SETUP_TIMING")) != 0;
    double stageT0 = nowMs();
    auto stage = [&](const char* what) {
        if (!stageTiming) return;
        const double t = nowMs();
        std::fprintf(stderr, "qgd_device_create: %-44s %8.2f s\n", what, (t - stageT0) * 1e-3);
        stageT0 = t;
    };
    StaticData s = buildStaticData(m);
    stage("static tables on the host (buildStaticData)");
    qgd_device_s* d = new qgd_device_s();
    try {
        d->deviceId = deviceId;
        d->nGeomD = m.nGeometricD;
        d->hasTri = s.hasTri;
        d->wedgePrism = hasWedgeAndPrism(m);
        d->patches = m.patches;
        residentCasePatchCheck(m, d->caseRefusal, d->caseRefusalCode);
        d->hf.assign(s.hf.begin(), s.hf.end());
        d->sensorRatio.resize((size_t)m.nFaces);
#pragma omp parallel for schedule(static)
        for (int64_t f = 0; f < m.nFaces; ++f) {
            // internal: nonOrthDeltaCoeffs / deltaCoeffs; patch: the patch snGrad coefficient (HostMesh::deltaCoeffs there) times |Cf - C_O|
            double r = -1.0;
            if (f < m.nInternalFaces) r = m.nonOrthDeltaCoeffs[f] / m.deltaCoeffs[f];
            else if (s.fkind[f] != FK_SKIP) {
                double d2 = 0;
                for (int k = 0; k < 3; ++k) { const double x = m.Cf[3 * (size_t)f + k] - m.C[3 * (size_t)m.owner[f] + k]; d2 += x * x; }
                r = m.deltaCoeffs[f] * std::sqrt(d2);
            }
            d->sensorRatio[f] = r;
        }
        const bool range = m.ownedEnd > m.ownedBegin;
        d->ownedBegin = range ? m.ownedBegin : 0;
        d->ownedEnd = range ? m.ownedEnd : m.nCells;
        d->cellGlobal = m.cellGlobal;
        d->cellGlobalOffset = m.cellGlobalOffset;
        for (int32_t c = 0; c < m.nCells && !m.cellIsGhost.empty(); ++c)
            if ((m.cellIsGhost[c] != 0) == (c >= d->ownedBegin && c < d->ownedEnd))
                throw std::invalid_argument("qgd_device_create: the owned cells of a shard must be one contiguous label range");
        HIP_CHECK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        DeviceArena& a = d->arena;
        MeshView& v = d->view;
        v.nP = s.nP; v.nF = s.nF; v.nIF = s.nIF; v.nC = s.nC; v.nBF = s.nBF;
        v.ie1 = s.ie1; v.ie2 = s.ie2; v.ie3 = s.ie3;
        v.nGeomD = m.nGeometricD;
        for (int k = 0; k < 3; ++k) v.emptyDir[k] = m.geometricD[k] < 0 ? 1 : 0;
        static const int kBlocks[] = {64, 128, 256};
        v.xcdRun = envChoice("QGD_XCD_RUN", 16, nullptr, 0, 0, 1 << 20);   // 0: one contiguous eighth of the tiles per XCD
        v.fuXcdRun = envChoice("QGD_FU_XCD_RUN", 64, nullptr, 0, 0, 1 << 20);   // (measured at 64 M cells: 4: 9.63, 16: 9.51-9.53, 64: 9.44, 256: 9.35-9.38 on one box; 16: 9.39, 64: 9.29-9.36, 1024: 9.38 on another)
        v.fblock = envChoice("QGD_FBLOCK", 128, kBlocks, 3);
        v.hasOther = 0;
        for (int64_t f = 0; f < s.nIF; ++f) if (s.fkind[f] == FK_OTHER) { v.hasOther = 1; break; }
        // Sf of a quadrilateral = (p3-p1) x (p4-p2) / 2 exactly (the triangle fan about any centre sums to it), and the
        // kernel holds those differences already: 24 B per face less to stream.  Not when the caller supplied its own Sf.
        v.sGeo = (envOnOff("QGD_SGEO", 1) != 0 && !m.userGeometry && v.fblock == 128) ? 1 : 0;
        // upload + free each table in turn so the host peak stays at one table
        auto up = [&](auto& vec) { auto* p = a.upload(vec); std::decay_t<decltype(vec)>().swap(vec); return p; };
        {
            // face tiles of the LDS-staged 3-D GaussVolPoint kernel (QGD_FTILE=0: the gather kernel)
            const char* e = std::getenv("QGD_FTILE");
            FaceTiles t;
            if (!e || std::atoi(e) != 0) t = buildFaceTiles(s, v.fblock);
            const int64_t lds = ((int64_t)t.maxCells * 104 + (int64_t)t.maxVerts * 72 + 255) / 256 * 256;
            // a numbering under which a quarter of the tiles do not fit (reverse Cuthill-McKee levels, scrambled labels) is
            // better off with the gather kernel alone: 2.68 instead of 2.97 ms on the 16 M-cell irregular mesh in RCM order
            const int64_t nTiles = t.fb ? (s.nIF + t.fb - 1) / t.fb : 0;
            if (t.fb != 0 && lds <= 65536 && 4 * (int64_t)t.spill.size() <= nTiles) {
                v.tileLds = (int32_t)lds;
                v.tileMaxC = t.maxCells; v.tileMaxV = t.maxVerts;
                v.qhdTiles = (uint16_t)envOnOff("QGD_QHD_TILES", 1);
                v.implTiles = (uint16_t)envOnOff("QGD_IMPL_TILES", 1);
                if (v.fblock == 128 && envOnOff("QGD_FTILE_FIXED", 1) != 0 &&
                    (int64_t)nTiles * std::max(t.maxCells, t.maxVerts) < (int64_t)INT32_MAX) {
                    // the lists once more at a fixed stride (built and uploaded one after the other: the host peak stays at one table)
                    std::vector<uint8_t> flag((size_t)nTiles, 0);
                    for (int32_t tile : t.spill) flag[tile] = 1;
                    auto padded = [&](const std::vector<int32_t>& list, int which, int32_t stride) {
                        std::vector<int32_t> out((size_t)nTiles * stride, 0);
#pragma omp parallel for schedule(static)
                        for (int64_t tile = 0; tile < nTiles; ++tile) {
                            const int32_t b = t.off[2 * tile + which], e = t.off[2 * (tile + 1) + which];
                            if (e == b) continue;
                            int32_t* o = out.data() + (size_t)tile * stride;
                            for (int32_t i = 0; i < stride; ++i) o[i] = list[b + std::min(i, e - b - 1)];
                        }
                        return out;
                    };
                    { auto pc = padded(t.cells, 0, t.maxCells); v.tileCellsFix = up(pc); }
                    { auto pv = padded(t.verts, 1, t.maxVerts); v.tileVertsFix = up(pv); }
                    v.tileFlag = up(flag);
                }
                v.nTileSpill = (int32_t)t.spill.size(); v.tileSpill = up(t.spill);
                v.tileOff = up(t.off); v.tileCells = up(t.cells); v.tileVerts = up(t.verts);
                v.locC = up(t.locC); v.locV = reinterpret_cast<const uint2*>(up(t.locV));
            }
        }
        {
            // cell blocks of the fused face + cell kernel (QGD_FUSED, qgd_setup.hpp FusedBlocks): 3-D unsharded meshes whose tiles were built
            static const int kFusedModes[] = {0, 1, 2};
            // 2: whatever the blocks look like (tests, probes); the caller's explicit choice (qgd_device_create_with) wins over the environment
            const int fusedMode = fusedChoice >= 0 ? fusedChoice : envChoice("QGD_FUSED", 1, kFusedModes, 3);
            if (fusedMode != 0) {
                stage("face tiles (build + upload)");
                FusedBlocks fb = buildFusedBlocks(s, false);   // (a mesh whose vertex weights pack keeps the 16-bit table alone)
                stage("cell blocks of the fused step (build)");
                int64_t owned = 0;
                for (int64_t ci = 0; ci < s.nC; ++ci) owned += (s.ghost.empty() || s.ghost[ci] != 1) ? 1 : 0;
                // what one workgroup may ask for without raising the kernel's dynamic-LDS attribute: the device's own figure (64 KB on gfx950)
                hipDeviceProp_t prop;
                HIP_CHECK(hipGetDeviceProperties(&prop, deviceId));
                const int64_t ldsLimit = std::min<int64_t>((int64_t)prop.sharedMemPerBlock, 64 * 1024);
                const FusedLaunchPlan plan = planFusedLaunch(fb, owned, ldsLimit, fusedMode == 2);   // (the rule and the LDS sizes: qgd_setup.hpp)
                if (plan.use) {
                    v.fuBlocks = fb.nBlocks; v.fuLayerBlocks = fb.nLayerBlocks; v.fuCapC = fb.capC; v.fuCapV = fb.capV; v.fuCapF = fb.capF;
                    v.fuCapE = fb.capE; v.fuLds = plan.lds; v.fuLdsCell = plan.ldsCell;
                    v.fuLdsImpl = plan.ldsImpl; v.fuLdsCellImpl = plan.ldsCellImpl;   // (the implicitDiffusion branch's layout of the same blocks)
                    v.fuCapPE = fb.capPE; v.fuMaxTot = (uint16_t)fb.maxTot; v.fuMaxAll = (uint16_t)fb.maxAll; v.fuMaxV = (uint16_t)fb.maxV; v.fuMaxF = (uint16_t)fb.maxF;   // (all within the caps checked above)
                    d->fusedFacesComputed = fb.facesComputed; d->fusedCellsStaged = fb.cellsStaged; d->fusedCellsStagedFull = fb.cellsStagedFull;
                    d->fusedVertsStaged = fb.vertsStaged;
                    v.fuHdr2 = reinterpret_cast<const int4*>(up(fb.hdr2)); v.fuVCount = up(fb.vCount); v.fuVPos = up(fb.vPos);
                    // the vertex weights: 16-bit offsets from one pattern where the mesh's weights pack (FusedBlocks::vW16), the doubles otherwise
                    if (fb.packedW) { v.fuVW = nullptr; v.fuVW16 = up(fb.vW16); v.fuVWRef = fb.wRef; }
                    else { v.fuVW = up(fb.vW); v.fuVW16 = nullptr; v.fuVWRef = 0; }
                    // the per-face streams w / hQGDf / kind, block-major as 16-bit offsets + a byte where they pack too (FusedBlocks::fW16)
                    v.fuFace = nullptr;
                    if (fb.packedF) {
                        FusedFaceView ff{};
                        ff.fuFW16 = up(fb.fW16); ff.fuFKC = up(fb.fKC); ff.fuFWRef = fb.fwRef;
                        for (int q = 0; q < 4; ++q) ff.fuFHRef[q] = fb.fhRef[q];
                        // (the geometry's view directly behind it, where that packs too: FusedBlocks::gCode)
                        FusedGeoView fg{};
                        if (fb.packedG) {
                            fg.fuGCode = up(fb.gCode); fg.fuGOwn = up(fb.gOwn); fg.fuGDict = up(fb.gDict); fg.fuGVRef = fb.gvRef; fg.fuGHRef = fb.ghRef;
                            v.fuGeo = 1;
                        }
                        std::vector<int64_t> raw((sizeof(FusedFaceView) + sizeof(FusedGeoView)) / 8);   // (uploaded as plain words)
                        std::memcpy(raw.data(), &ff, sizeof ff);
                        std::memcpy(raw.data() + sizeof ff / 8, &fg, sizeof fg);
                        v.fuFace = reinterpret_cast<const FusedFaceView*>(up(raw));
                    }
                    v.fuHdr = reinterpret_cast<const int4*>(up(fb.hdr)); v.fuCells = up(fb.cells); v.fuVerts = up(fb.verts);
                    v.fuFaceLabel = up(fb.faceLabel); v.fuFacePos = up(fb.facePos); v.fuNEntry = up(fb.nEntry); v.fuEntry = up(fb.entry);
                    d->fusedInfo[0] = fb.nBlocks; d->fusedInfo[1] = fb.nLayerBlocks; d->fusedInfo[2] = fb.nTemplates; d->fusedInfo[3] = plan.lds;
                    // bytes a block streams per step out of its own lists / of its template's
                    d->fusedInfo[4] = 32 + 4 * (int64_t)fb.capC + 4 * (int64_t)fb.capV + 4 * (int64_t)fb.capF + fb.capV + 128 + (fb.packedW ? 2 : 8) * (int64_t)fb.capPE * fb.capV +
                                      (fb.packedF ? 5 * (int64_t)fb.capF : 0) + (fb.packedG ? 256 * 16 + 128 * 4 + 96 * 8 : 0);
                    d->fusedInfo[5] = 12 * (int64_t)fb.capF + 4 * (int64_t)fb.capE * 128 + 2 * (int64_t)fb.capPE * fb.capV;
                    // (above the milliseconds' 32 bits: the largest geometry dictionary and the largest 12-bit offset, for tests and reports)
                    d->fusedInfo[6] = std::min<int64_t>((int64_t)(fb.buildSeconds * 1e3), 0xffffffffLL) | (int64_t)(fb.maxGeoDict & 31) << 32 | (int64_t)(fb.maxGeoOffset & 4095) << 40;
                    // (the figures above bit 25 say what the packed tables hold, for tests and reports: nothing reads them to decide anything)
                    d->fusedInfo[7] = fb.brick[0] | fb.brick[1] << 8 | fb.brick[2] << 16 | (fb.packedW ? 1 << 24 : 0) | (fb.packedF ? 1 << 25 : 0) |
                                      (int64_t)(fb.nHfClasses & 7) << 26 | (int64_t)(fb.maxWeightOffset & 0xffff) << 29 | (int64_t)(fb.maxFaceOffset & 0xffff) << 45 |
                                      (int64_t)(fb.packedG ? 1 : 0) << 61;
                }
            }
        }
        stage("block tables (upload) / up to the static tables");
        v.own = up(s.own); v.nei = up(s.nei);
        v.verts = reinterpret_cast<const int4*>(up(s.verts));
        v.fkind = up(s.fkind);
        v.Sx = up(s.Sf[0]); v.Sy = up(s.Sf[1]); v.Sz = up(s.Sf[2]);
        v.magSf = up(s.magSf); v.w = up(s.w); v.hf = up(s.hf); v.dn = up(s.dn);
        v.X = up(s.X); v.Cc = up(s.Cc);
        v.bN = reinterpret_cast<const double4*>(up(s.bN)); v.bmvON = up(s.bmvON);
        v.ip13 = reinterpret_cast<const int2*>(up(s.ip13)); v.c2d = up(s.c2d);
        v.lsqSlice = up(s.lsqSlice); v.lsqCnt = up(s.lsqCnt); v.lsqCell = up(s.lsqCell);
        v.lsqGx = up(s.lsqGx); v.lsqGy = up(s.lsqGy); v.lsqGz = up(s.lsqGz); v.lsqDeg = up(s.lsqDeg);
        v.lsqBndZero = up(s.lsqBndZero);
        if (!s.bSymm.empty()) v.bSymm = up(s.bSymm);
        v.pcSlice = up(s.pcSlice); v.pcCount = up(s.pcCount); v.pcCell = up(s.pcCell); v.pcW = up(s.pcW);
        v.nBP = (int32_t)s.bpPoint.size();
        v.bpPoint = up(s.bpPoint); v.bpOff = up(s.bpOff); v.bpFace = up(s.bpFace); v.bpW = up(s.bpW);
        if (!s.cpOff.empty() && s.cpOff.back() > 0) { v.cpOff = up(s.cpOff); v.cpKind = up(s.cpKind); v.cpT = up(s.cpT); }
        v.cfSlice = up(s.cfSlice); v.cfCount = up(s.cfCount); v.cfItem = up(s.cfItem); v.cfNbr = up(s.cfNbr);
        v.fpos = up(s.fpos); v.cfPos = up(s.cfPos);
        v.V = up(s.V); v.hQGD = up(s.hQGD); v.ghost = up(s.ghost);
        v.bPatch = up(s.bPatch); v.hQGDb = up(s.hQGDb);
        {
            // a cell on a shard corner is needed by several neighbours: once in the list the update kernel walks
            std::vector<int32_t> sc, sf;
            for (size_t slot = 0; slot < s.haloSend.size(); ++slot) {
                sc.insert(sc.end(), s.haloSend[slot].begin(), s.haloSend[slot].end());
                sf.insert(sf.end(), s.haloSendBF[slot].begin(), s.haloSendBF[slot].end());
            }
            std::sort(sc.begin(), sc.end()); sc.erase(std::unique(sc.begin(), sc.end()), sc.end());
            std::sort(sf.begin(), sf.end()); sf.erase(std::unique(sf.begin(), sf.end()), sf.end());
            d->nSendAll = (int32_t)sc.size(); d->nSendBFAll = (int32_t)sf.size();
            d->sendAll = a.upload(sc); d->sendBFAll = a.upload(sf);
        }
        d->haloSelf = m.haloSelf;
        if (!d->haloSelf.empty() && d->haloSelf.size() != s.haloGhost.size()) throw std::invalid_argument("qgd_device_create: haloSelf does not match the halo slots");
        d->halo.resize(s.haloGhost.size());
        for (size_t slot = 0; slot < d->halo.size(); ++slot) {
            qgd_device_s::HaloSlot& h = d->halo[slot];
            h.nGhost = (int32_t)s.haloGhost[slot].size();
            h.nSend = (int32_t)s.haloSend[slot].size();
            h.nGhostBF = (int32_t)s.haloGhostBF[slot].size();
            h.nSendBF = (int32_t)s.haloSendBF[slot].size();
            h.ghost = a.upload(s.haloGhost[slot]);
            h.send = a.upload(s.haloSend[slot]);
            h.ghostBF = a.upload(s.haloGhostBF[slot]);
            h.sendBF = a.upload(s.haloSendBF[slot]);
        }
    } catch (...) {
        d->arena.release();
        if (d->stream) (void)hipStreamDestroy(d->stream);
        delete d;
        throw;
    }
    stage("static tables (upload), halo lists");
    *out = d;
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_create(qgd_mesh_t mh, int deviceId, qgd_device_t* out) { return deviceCreate(mh, deviceId, -1, out); }
int qgd_device_create_with(qgd_mesh_t mh, int deviceId, int32_t flags, qgd_device_t* out) {
    if (flags & ~(QGD_DEVICE_NO_FUSED_TABLES | QGD_DEVICE_FUSED_ANY_BLOCKS)) return fail(QGD_ERR_INVALID, "qgd_device_create_with: unknown flag");
    if ((flags & QGD_DEVICE_NO_FUSED_TABLES) && (flags & QGD_DEVICE_FUSED_ANY_BLOCKS))
        return fail(QGD_ERR_INVALID, "qgd_device_create_with: QGD_DEVICE_NO_FUSED_TABLES and QGD_DEVICE_FUSED_ANY_BLOCKS exclude each other");
    return deviceCreate(mh, deviceId, (flags & QGD_DEVICE_NO_FUSED_TABLES) ? 0 : ((flags & QGD_DEVICE_FUSED_ANY_BLOCKS) ? 2 : -1), out);
}
int qgd_device_free(qgd_device_t d) {
    if (!d) return QGD_OK;
    // a case keeps a pointer to its device and runs on its stream: freed after the device it would read freed memory
    if (d->liveCases > 0)
        return fail(QGD_ERR_INVALID, "qgd_device_free: " + std::to_string(d->liveCases) + " case(s) created on this device are still open; free them first");
    (void)hipSetDevice(d->deviceId);
    if (d->opSolver) { (void)hipStreamSynchronize(d->stream); implicitSolverFree(d->opSolver); d->opSolver = nullptr; }
    d->ws.release();
    for (hipEvent_t e : d->opEv) if (e) (void)hipEventDestroy(e);
    d->arena.release();
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return QGD_OK;
}

static const char* kWedgePrismMessage =
    "GaussVolPoint scheme does not support solving axisymmetric cases with wedge BC and prism cells. Try to set leastSquares scheme.";

// fvscOpName + fvscStencil::New [fvsc_8C L47-85, fvscStencil_8C L59-95]
static int stencilWordToId(int nGeomD, const std::string& w, int* id) {
    if ((w == "leastSquares" || w == "leastSquaresOpt") && nGeomD == 3)
        return fail(QGD_ERR_SCHEME, "Can't use leastSquares or leastSquaresOpt in 3D case.");
    if (w == "reduced") *id = QGD_FVSC_REDUCED;
    else if (w == "leastSquares" || w == "leastSquaresOpt") *id = QGD_FVSC_LEASTSQUARES;
    else if (w == "GaussVolPoint") *id = QGD_FVSC_GAUSSVOLPOINT;
    else return fail(QGD_ERR_UNKNOWN_NAME, "Unknown Model type " + w + "; valid: GaussVolPoint leastSquares leastSquaresOpt reduced");
    return QGD_OK;
}
static int deviceStencilRaw(int nGeomD, int id, int* st) {
    if (id == QGD_FVSC_REDUCED) *st = ST_REDUCED;
    else if (id == QGD_FVSC_LEASTSQUARES) {
        if (nGeomD == 3) return fail(QGD_ERR_SCHEME, "Can't use leastSquares or leastSquaresOpt in 3D case.");
        *st = ST_LSQ;
    } else if (id == QGD_FVSC_GAUSSVOLPOINT) *st = (nGeomD == 3) ? ST_GVP3 : (nGeomD == 2 ? ST_GVP2 : ST_REDUCED);
    else return fail(QGD_ERR_UNKNOWN_NAME, "bad stencil id");
    return QGD_OK;
}
static int deviceStencil(const qgd_device_s* d, int id, int* st) {
    if (d->wedgePrism && id == QGD_FVSC_GAUSSVOLPOINT) return fail(QGD_ERR_SCHEME, kWedgePrismMessage);
    return deviceStencilRaw(d->nGeomD, id, st);
}
int qgd_stencil_lookup(qgd_device_t d, const char* word, int* stencilId) {
    if (!d || !word || !stencilId) return fail(QGD_ERR_INVALID, "null argument");
    if (d->wedgePrism && std::string(word) == "GaussVolPoint") return fail(QGD_ERR_SCHEME, kWedgePrismMessage);
    return stencilWordToId(d->nGeomD, word, stencilId);
}

// whether `name` ends in ".boundary", which is stripped
static bool boundaryName(std::string& name) {
    const std::string suffix = ".boundary";
    if (name.size() <= suffix.size() || name.compare(name.size() - suffix.size(), suffix.size(), suffix) != 0) return false;
    name.resize(name.size() - suffix.size());
    return true;
}
// `count` faces of `nc` components, SoA with stride `count` on the device, to `nc` per face at the caller: one transposition (WS_XPOSE), one copy
static void fetchFaceSoA(qgd_device_s* d, hipStream_t stream, const double* src, int64_t count, int nc, double* out) {
    if (nc == 1) { d->ws.d2h(out, src, sizeof(double) * (size_t)count, stream); return; }
    double* tmp = d->ws.get<double>(WS_XPOSE, (size_t)count * nc);
    launchSoaToAos(stream, count, nc, src, tmp);
    HIP_CHECK(hipGetLastError());
    d->ws.d2h(out, tmp, sizeof(double) * (size_t)count * nc, stream);
}
static int fvscOp(qgd_device_t d, int stencilId, int op, int NC, const double* cell, const double* bnd, double* out) {
    QGD_TRY
    if (!d || !cell || !out || (!bnd && d->view.nBF > 0)) return fail(QGD_ERR_INVALID, "fvsc operator: null argument");
    int st = 0;
    int rc = deviceStencil(d, stencilId, &st);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    const int NO = (op == 0) ? 3 * NC : NC / 3;
    Workspace& ws = d->ws;
    double* dc = ws.get<double>(WS_CELL, (size_t)v.nC * NC);
    double* db = ws.get<double>(WS_BND, (size_t)v.nBF * NC);
    double* dp = ws.get<double>(WS_PT, (size_t)v.nP * NC);
    double* dout = ws.get<double>(WS_OUT, (size_t)v.nF * NO);
    if (!d->opEv[0]) { HIP_CHECK(hipEventCreate(&d->opEv[0])); HIP_CHECK(hipEventCreate(&d->opEv[1])); }
    const double t0 = nowMs();
    ws.h2d(dc, cell, sizeof(double) * (size_t)v.nC * NC, d->stream);
    if (v.nBF) ws.h2d(db, bnd, sizeof(double) * (size_t)v.nBF * NC, d->stream);
    HIP_CHECK(hipMemsetAsync(dp, 0, sizeof(double) * (size_t)v.nP * NC, d->stream));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    const double t1 = nowMs();
    (void)hipGetLastError();  // drop any stale sticky error so the check below is about our launches
    HIP_CHECK(hipEventRecord(d->opEv[0], d->stream));
    launchFvscOp(d->stream, st, op, NC, v, dc, db, dp, dout);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(d->opEv[1], d->stream));
    HIP_CHECK(hipEventSynchronize(d->opEv[1]));
    const double t2 = nowMs();
    ws.d2h(out, dout, sizeof(double) * (size_t)v.nF * NO, d->stream);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    float kms = 0;
    (void)hipEventElapsedTime(&kms, d->opEv[0], d->opEv[1]);
    d->opMs[0] = t1 - t0; d->opMs[1] = kms; d->opMs[2] = nowMs() - t2;
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_op_times(qgd_device_t d, double ms[3]) {
    if (!d || !ms) return fail(QGD_ERR_INVALID, "null argument");
    for (int k = 0; k < 3; ++k) ms[k] = d->opMs[k];
    return QGD_OK;
}
int qgd_device_face_tiles(qgd_device_t d, int64_t info[4]) {
    if (!d || !info) return fail(QGD_ERR_INVALID, "null argument");
    const MeshView& v = d->view;
    const bool on = v.tileOff != nullptr;
    info[0] = on ? v.fblock : 0;
    info[1] = on ? (v.nIF + v.fblock - 1) / v.fblock : 0;
    info[2] = on ? v.nTileSpill : 0;
    info[3] = on ? v.tileLds : 0;
    return QGD_OK;
}
int qgd_device_fused_blocks(qgd_device_t d, int64_t info[8]) {
    if (!d || !info) return fail(QGD_ERR_INVALID, "null argument");
    for (int k = 0; k < 8; ++k) info[k] = d->fusedInfo[k];
    return QGD_OK;
}
int qgd_fvsc_grad_s(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOp(d, id, 0, 1, cell, bnd, out); }
int qgd_fvsc_grad_v(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOp(d, id, 0, 3, cell, bnd, out); }
int qgd_fvsc_div_v(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOp(d, id, 1, 3, cell, bnd, out); }
int qgd_fvsc_div_t(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOp(d, id, 1, 9, cell, bnd, out); }

// ---- the same operators on DEVICE pointers: no staging, no PCIe, stream-ordered on the device handle's stream ----------------
// (a level-1 adapter whose fields already live in HBM -- another GPU library, a device-resident OpenFOAM build -- pays the
// kernels only: ~3 ms instead of ~80 ms per four gradients at 8 M cells)
static int fvscOpDev(qgd_device_t d, int stencilId, int op, int NC, const double* cell, const double* bnd, double* out) {
    QGD_TRY
    if (!d || !cell || !out || (!bnd && d->view.nBF > 0)) return fail(QGD_ERR_INVALID, "fvsc operator (device pointers): null argument");
    int st = 0;
    int rc = deviceStencil(d, stencilId, &st);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    double* dp = d->ws.get<double>(WS_PT, (size_t)v.nP * NC);   // vertex values: the one work array (grow-only, reused)
    HIP_CHECK(hipMemsetAsync(dp, 0, sizeof(double) * (size_t)v.nP * NC, d->stream));
    (void)hipGetLastError();
    launchFvscOp(d->stream, st, op, NC, v, cell, bnd, dp, out);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
    QGD_CATCH
}
int qgd_fvsc_grad_s_dev(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOpDev(d, id, 0, 1, cell, bnd, out); }
int qgd_fvsc_grad_v_dev(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOpDev(d, id, 0, 3, cell, bnd, out); }
int qgd_fvsc_div_v_dev(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOpDev(d, id, 1, 3, cell, bnd, out); }
int qgd_fvsc_div_t_dev(qgd_device_t d, int id, const double* cell, const double* bnd, double* out) { return fvscOpDev(d, id, 1, 9, cell, bnd, out); }
int qgd_interpolate_dev(qgd_device_t d, int32_t ncomp, const double* cell, const double* bnd, double* out) {
    QGD_TRY
    if (!d || !cell || !out || ncomp < 1 || ncomp > 9 || (!bnd && d->view.nBF > 0)) return fail(QGD_ERR_INVALID, "qgd_interpolate_dev: bad argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    (void)hipGetLastError();
    launchInterpolate(d->stream, ncomp, d->view, cell, bnd, out);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_sync(qgd_device_t d) {
    QGD_TRY
    if (!d) return fail(QGD_ERR_INVALID, "null device");
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
// the leastSquares stencil of an internal face as the device holds it (sliced ELL read back): cells in the order they are summed
int qgd_device_lsq_stencil(qgd_device_t d, int32_t face, int32_t* cells, int32_t cap, int32_t* count) {
    QGD_TRY
    if (!d || !count || (cap > 0 && !cells)) return fail(QGD_ERR_INVALID, "qgd_device_lsq_stencil: bad argument");
    const MeshView& m = d->view;
    if (!m.lsqCnt || !m.lsqSlice || !m.lsqCell) return fail(QGD_ERR_SCHEME, "qgd_device_lsq_stencil: the mesh has no leastSquares stencil (3-D)");
    if (face < 0 || face >= m.nIF) return fail(QGD_ERR_INVALID, "qgd_device_lsq_stencil: not an internal face");
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    uint8_t cnt8 = 0;
    int32_t slice = 0;
    HIP_CHECK(hipMemcpy(&cnt8, m.lsqCnt + face, sizeof(uint8_t), hipMemcpyDeviceToHost));
    const int32_t cnt = cnt8;
    HIP_CHECK(hipMemcpy(&slice, m.lsqSlice + (face >> 6), sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int k = 0; k < cnt && k < cap; ++k)
        HIP_CHECK(hipMemcpy(cells + k, m.lsqCell + ((size_t)slice + k) * 64 + (face & 63), sizeof(int32_t), hipMemcpyDeviceToHost));
    *count = cnt;
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_copy(qgd_device_t d, void* dst, const void* src, int64_t bytes, int toDevice) {
    QGD_TRY
    if (!d || !dst || !src || bytes < 0) return fail(QGD_ERR_INVALID, "qgd_device_copy: bad argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    // on the device's own stream and complete at return: that stream is non-blocking, and a hipMemcpy from pageable memory on the null
    // stream may return while its staged copy is still on the way -- a kernel queued on d->stream right after could read the old bytes
    if (bytes) HIP_CHECK(hipMemcpyAsync(dst, src, (size_t)bytes, toDevice ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, d->stream));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
// ---- QHDFoam face fluxes -------------------------------------------------------------
// what both entries refuse (`who`: the entry the caller called); the same questions of host and of device pointers
static int qhdFluxesCheck(qgd_device_t d, const std::string& who, int stencilId, const qgd_qhd_inputs* in, const qgd_qhd_outputs* out, int* st) {
    if (!d || !in || !out) return fail(QGD_ERR_INVALID, who + ": null argument");
    const MeshView& v = d->view;
    if (!in->U || !in->T || !in->rho || !in->tauQGDf || (v.nBF > 0 && (!in->Ub || !in->Tb || !in->rhob)))
        return fail(QGD_ERR_INVALID, who + ": U, T, rho (cell + patch values) and tauQGDf are required");
    const bool haveP = in->p != nullptr;
    if (haveP && v.nBF > 0 && !in->pb) return fail(QGD_ERR_INVALID, who + ": p given without its patch values");
    if ((out->gradPf || out->Wf || out->phiUf) && !haveP) return fail(QGD_ERR_INVALID, who + ": gradPf/Wf/phiUf need p");
    if ((out->phiUf || out->phiTf) && !in->phi) return fail(QGD_ERR_INVALID, who + ": phiUf/phiTf need phi");
    return deviceStencil(d, stencilId, st);
}
// every output from inputs on the device, as the SoA block of launchQhdFluxes (QHD_COUNT slots of nF doubles in WS_OUT)
static const double* qhdFluxesFill(qgd_device_t d, int st, const qgd_qhd_inputs* in) {
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    const bool haveP = in->p != nullptr;
    const size_t nC = (size_t)v.nC, nB = (size_t)v.nBF, nF = (size_t)v.nF, nP = (size_t)v.nP;
    Workspace& ws = d->ws;
    hipStream_t s_ = d->stream;
    double* dCell = ws.get<double>(WS_CELL, 5 * nC);
    double* dBnd = ws.get<double>(WS_BND, 5 * std::max<size_t>(nB, 1));
    double* dPt = ws.get<double>(WS_PT, 5 * nP);
    double* dOut = ws.get<double>(WS_OUT, (size_t)QHD_COUNT * nF);
    (void)hipGetLastError();
    launchPack5(s_, (int64_t)nC, in->U, in->T, in->p, dCell);
    launchPack5(s_, (int64_t)nB, in->Ub, in->Tb, haveP ? in->pb : nullptr, dBnd);
    HIP_CHECK(hipMemsetAsync(dPt, 0, sizeof(double) * std::max<size_t>(5 * nP, 1), s_));
    HIP_CHECK(hipMemsetAsync(dOut, 0, sizeof(double) * (size_t)QHD_COUNT * nF, s_));
    launchQhdFluxes(s_, st, v, dCell, dBnd, dPt, in->rho, in->rhob, in->tauQGDf, in->phi, in->beta, in->g[0], in->g[1], in->g[2], dOut);
    HIP_CHECK(hipGetLastError());
    return dOut;
}
// every output of the block: its pointer in qgd_qhd_outputs, first slot, components
static const struct { double* qgd_qhd_outputs::*dst; int first, nc; } kQhdOutputs[] = {
    {&qgd_qhd_outputs::gradUf, QHD_GRADU, 9}, {&qgd_qhd_outputs::gradTf, QHD_GRADT, 3}, {&qgd_qhd_outputs::phiu, QHD_PHIU, 1},
    {&qgd_qhd_outputs::phiwo, QHD_PHIWO, 1}, {&qgd_qhd_outputs::taubyrhof, QHD_TAUBYRHO, 1}, {&qgd_qhd_outputs::gradPf, QHD_GRADP, 3},
    {&qgd_qhd_outputs::Wf, QHD_WF, 3}, {&qgd_qhd_outputs::phiUf, QHD_PHIUF, 3}, {&qgd_qhd_outputs::phiTf, QHD_PHITF, 1},
    {&qgd_qhd_outputs::phiTauTReg, QHD_PHITAUT, 1}};
// qgd_qhd_fluxes on device pointers; outputs in the documented face-major layout
int qgd_qhd_fluxes_dev(qgd_device_t d, int stencilId, const qgd_qhd_inputs* in, qgd_qhd_outputs* out) {
    QGD_TRY
    int st = 0;
    const int rc = qhdFluxesCheck(d, "qgd_qhd_fluxes_dev", stencilId, in, out, &st);
    if (rc) return rc;
    const double* dOut = qhdFluxesFill(d, st, in);
    const size_t nF = (size_t)d->view.nF;
    for (const auto& o : kQhdOutputs)
        if (out->*o.dst) launchSoaToAos(d->stream, (int64_t)nF, o.nc, dOut + (size_t)o.first * nF, out->*o.dst);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
    QGD_CATCH
}
// the same on host pointers: the caller's arrays are staged as they are (the records are packed on the device), and each requested output
// comes back through the one transposition slot -- never all ten face-major outputs on the device at once
int qgd_qhd_fluxes(qgd_device_t d, int stencilId, const qgd_qhd_inputs* in, qgd_qhd_outputs* out) {
    QGD_TRY
    int st = 0;
    const int rc = qhdFluxesCheck(d, "qgd_qhd_fluxes", stencilId, in, out, &st);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const size_t nC = (size_t)d->view.nC, nB = (size_t)d->view.nBF, nF = (size_t)d->view.nF;
    Stager stage{d->ws, d->stream};
    qgd_qhd_inputs din = *in;
    din.U = stage.up(in->U, 3 * nC); din.Ub = stage.up(in->Ub, 3 * nB);
    din.T = stage.up(in->T, nC); din.Tb = stage.up(in->Tb, nB);
    if (in->p) { din.p = stage.up(in->p, nC); din.pb = stage.up(in->pb, nB); }
    din.rho = stage.up(in->rho, nC); din.rhob = stage.up(in->rhob, nB);
    din.tauQGDf = stage.up(in->tauQGDf, nF);
    if (in->phi) din.phi = stage.up(in->phi, nF);
    const double* dOut = qhdFluxesFill(d, st, &din);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    for (const auto& o : kQhdOutputs)
        if (out->*o.dst) fetchFaceSoA(d, d->stream, dOut + (size_t)o.first * nF, (int64_t)nF, o.nc, out->*o.dst);
    return QGD_OK;
    QGD_CATCH
}

// ---- species flux and step -------------------------------------------------------------
// As for the QHD fluxes: what both entries refuse (`who`: the entry called), asked of host or of device pointers before any device work; then
// the launches on device pointers.
static int speciesFluxCheck(qgd_device_t d, const std::string& who, int stencilId, const double* Y, const double* Yb, const double* U, const double* Ub,
                            const double* phiJm, const double* phi, const double* tauQGDf, const double* phiJmY, const double* diffusiveFlux, int* st) {
    if (!d || !Y || !U || !phiJm || !phi || !tauQGDf || !phiJmY || !diffusiveFlux)
        return fail(QGD_ERR_INVALID, who + ": null argument");
    if (d->view.nBF > 0 && (!Yb || !Ub)) return fail(QGD_ERR_INVALID, who + ": patch values of Y and U are required");
    return deviceStencil(d, stencilId, st);
}
static void speciesFluxRun(qgd_device_t d, int st, const double* Y, const double* Yb, const double* U, const double* Ub, const double* phiJm,
                           const double* phi, const double* tauQGDf, double* phiJmY, double* diffusiveFlux, double* gradYf) {
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    const size_t nF = (size_t)v.nF, nP = (size_t)v.nP;
    hipStream_t s_ = d->stream;
    double* dPt = d->ws.get<double>(WS_PT, nP);
    double* dOut = d->ws.get<double>(WS_OUT, 5 * nF);
    HIP_CHECK(hipMemsetAsync(dPt, 0, sizeof(double) * std::max<size_t>(nP, 1), s_));
    (void)hipGetLastError();
    launchSpeciesFlux(s_, st, v, Y, Yb, dPt, U, Ub, phiJm, phi, tauQGDf, dOut);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(phiJmY, dOut, sizeof(double) * nF, hipMemcpyDeviceToDevice, s_));
    HIP_CHECK(hipMemcpyAsync(diffusiveFlux, dOut + nF, sizeof(double) * nF, hipMemcpyDeviceToDevice, s_));
    if (gradYf) launchSoaToAos(s_, (int64_t)nF, 3, dOut + 2 * nF, gradYf);
    HIP_CHECK(hipGetLastError());
}
int qgd_species_flux_dev(qgd_device_t d, int stencilId, const double* Y, const double* Yb, const double* U, const double* Ub,
                         const double* phiJm, const double* phi, const double* tauQGDf, double* phiJmY, double* diffusiveFlux,
                         double* gradYf) {
    QGD_TRY
    int st = 0;
    const int rc = speciesFluxCheck(d, "qgd_species_flux_dev", stencilId, Y, Yb, U, Ub, phiJm, phi, tauQGDf, phiJmY, diffusiveFlux, &st);
    if (rc) return rc;
    speciesFluxRun(d, st, Y, Yb, U, Ub, phiJm, phi, tauQGDf, phiJmY, diffusiveFlux, gradYf);
    return QGD_OK;
    QGD_CATCH
}
int qgd_species_flux(qgd_device_t d, int stencilId, const double* Y, const double* Yb, const double* U, const double* Ub,
                     const double* phiJm, const double* phi, const double* tauQGDf, double* phiJmY, double* diffusiveFlux,
                     double* gradYf) {
    QGD_TRY
    int st = 0;
    const int rc = speciesFluxCheck(d, "qgd_species_flux", stencilId, Y, Yb, U, Ub, phiJm, phi, tauQGDf, phiJmY, diffusiveFlux, &st);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const size_t nC = (size_t)d->view.nC, nB = (size_t)d->view.nBF, nF = (size_t)d->view.nF;
    Stager stage{d->ws, d->stream};
    double *dY = stage.up(Y, nC), *dYb = stage.up(Yb, nB), *dU = stage.up(U, 3 * nC), *dUb = stage.up(Ub, 3 * nB);
    double *dJm = stage.up(phiJm, nF), *dPhi = stage.up(phi, nF), *dTau = stage.up(tauQGDf, nF);
    double *dJmY = stage.scratch(nF), *dDf = stage.scratch(nF), *dGrad = gradYf ? stage.scratch(3 * nF) : nullptr;
    speciesFluxRun(d, st, dY, dYb, dU, dUb, dJm, dPhi, dTau, dJmY, dDf, dGrad);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    d->ws.d2h(phiJmY, dJmY, sizeof(double) * nF, d->stream);
    d->ws.d2h(diffusiveFlux, dDf, sizeof(double) * nF, d->stream);
    if (gradYf) d->ws.d2h(gradYf, dGrad, sizeof(double) * 3 * nF, d->stream);
    return QGD_OK;
    QGD_CATCH
}

static int speciesStepCheck(qgd_device_t d, const std::string& who, const double* Y, const double* Yb, const double* rhoOld, const double* rho,
                            const double* phiJmY, const double* muf, double Sc, double deltaT, const double* diffusiveFlux, const double* Ynew) {
    if (!d || !Y || !rhoOld || !rho || !phiJmY || !muf || !diffusiveFlux || !Ynew) return fail(QGD_ERR_INVALID, who + ": null argument");
    if (!(Sc > 0) || !(deltaT > 0)) return fail(QGD_ERR_INVALID, who + ": Sc and deltaT must be positive");
    if (d->view.nBF > 0 && !Yb) return fail(QGD_ERR_INVALID, who + ": patch values of Y are required");
    return QGD_OK;
}
static void speciesStepRun(qgd_device_t d, const double* Y, const double* Yb, const double* rhoOld, const double* rho, const double* phiJmY,
                           const double* muf, double Sc, double deltaT, const double* Su, double* diffusiveFlux, double* Ynew) {
    HIP_CHECK(hipSetDevice(d->deviceId));
    double* net = d->ws.get<double>(WS_OUT, (size_t)d->view.nF);
    (void)hipGetLastError();
    launchSpeciesStep(d->stream, d->view, Y, Yb, rhoOld, rho, phiJmY, muf, Sc, deltaT, Su, diffusiveFlux, net, Ynew);
    HIP_CHECK(hipGetLastError());
}
int qgd_species_step_dev(qgd_device_t d, const double* Y, const double* Yb, const double* rhoOld, const double* rho, const double* phiJmY,
                         const double* muf, double Sc, double deltaT, const double* Su, double* diffusiveFlux, double* Ynew) {
    QGD_TRY
    const int rc = speciesStepCheck(d, "qgd_species_step_dev", Y, Yb, rhoOld, rho, phiJmY, muf, Sc, deltaT, diffusiveFlux, Ynew);
    if (rc) return rc;
    speciesStepRun(d, Y, Yb, rhoOld, rho, phiJmY, muf, Sc, deltaT, Su, diffusiveFlux, Ynew);
    return QGD_OK;
    QGD_CATCH
}
int qgd_species_step(qgd_device_t d, const double* Y, const double* Yb, const double* rhoOld, const double* rho, const double* phiJmY,
                     const double* muf, double Sc, double deltaT, const double* Su, double* diffusiveFlux, double* Ynew) {
    QGD_TRY
    const int rc = speciesStepCheck(d, "qgd_species_step", Y, Yb, rhoOld, rho, phiJmY, muf, Sc, deltaT, diffusiveFlux, Ynew);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const size_t nC = (size_t)d->view.nC, nB = (size_t)d->view.nBF, nF = (size_t)d->view.nF;
    Stager stage{d->ws, d->stream};
    double *dY = stage.up(Y, nC), *dYb = stage.up(Yb, nB), *dRo = stage.up(rhoOld, nC), *dR = stage.up(rho, nC);
    double *dJ = stage.up(phiJmY, nF), *dMu = stage.up(muf, nF), *dSu = Su ? stage.up(Su, nC) : nullptr;
    double *dDf = stage.up(diffusiveFlux, nF), *dNew = stage.scratch(nC);
    speciesStepRun(d, dY, dYb, dRo, dR, dJ, dMu, Sc, deltaT, dSu, dDf, dNew);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    d->ws.d2h(diffusiveFlux, dDf, sizeof(double) * nF, d->stream);
    d->ws.d2h(Ynew, dNew, sizeof(double) * nC, d->stream);
    return QGD_OK;
    QGD_CATCH
}
// the implicitDiffusion branch of the species equation [QGDYEqn_8H L47-66] on device pointers; info (host) = {iterations, initial, final residual}
int qgd_species_step_implicit_dev(qgd_device_t d, const double* Y, const double* Yb, const uint8_t* fixedValueFace, const double* rhoOld,
                                  const double* rho, const double* phiJmY, const double* muf, double Sc, double deltaT, const double* Su, double tolerance,
                                  int32_t maxIter, double* diffusiveFlux, double* Ynew, double info[3]) {
    QGD_TRY
    if (!d || !Y || !rhoOld || !rho || !phiJmY || !muf || !diffusiveFlux || !Ynew || !info)
        return fail(QGD_ERR_INVALID, "qgd_species_step_implicit_dev: null argument");
    if (!(Sc > 0) || !(deltaT > 0) || !(tolerance > 0) || maxIter < 1)
        return fail(QGD_ERR_INVALID, "qgd_species_step_implicit_dev: Sc, deltaT, tolerance must be positive, maxIter >= 1");
    const MeshView& v = d->view;
    if (v.nBF > 0 && !Yb) return fail(QGD_ERR_INVALID, "qgd_species_step_implicit_dev: patch values of Y are required");
    if (d->sharded()) return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_species_step_implicit: the stateless operator solves on one device (no reductions across shards)");
    for (const Patch& pt : d->patches)   // fvm::laplacian couples the two sides of a cyclic patch inside the matrix; this one has no such rows
        if (pt.type == QGD_PATCH_CYCLIC && pt.nonEmptyGlobally())
            return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_species_step_implicit: patch '" + pt.name + "' is cyclic: the implicit laplacian across coupled patches is not served");
    HIP_CHECK(hipSetDevice(d->deviceId));
    if (!d->opSolver) d->opSolver = implicitSolverCreate(d->stream, v, d->ownedBegin, d->ownedEnd);
    double* work = d->ws.get<double>(WS_H, 3 * (size_t)v.nC + (size_t)v.nF);
    (void)hipGetLastError();
    launchSpeciesStepImplicit(d->opSolver, v, Y, Yb, fixedValueFace, rhoOld, rho, phiJmY, muf, Sc, deltaT, Su, tolerance, maxIter, work, diffusiveFlux, Ynew, info);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
    QGD_CATCH
}
int qgd_species_step_implicit(qgd_device_t d, const double* Y, const double* Yb, const uint8_t* fixedValueFace, const double* rhoOld, const double* rho,
                              const double* phiJmY, const double* muf, double Sc, double deltaT, const double* Su, double tolerance, int32_t maxIter,
                              double* diffusiveFlux, double* Ynew, double info[3]) {
    QGD_TRY
    if (!d || !Y || !rhoOld || !rho || !phiJmY || !muf || !diffusiveFlux || !Ynew || !info)
        return fail(QGD_ERR_INVALID, "qgd_species_step_implicit: null argument");
    const MeshView& v = d->view;
    if (v.nBF > 0 && !Yb) return fail(QGD_ERR_INVALID, "qgd_species_step_implicit: patch values of Y are required");
    HIP_CHECK(hipSetDevice(d->deviceId));
    const size_t nC = (size_t)v.nC, nB = (size_t)v.nBF, nF = (size_t)v.nF;
    Workspace& ws = d->ws;
    hipStream_t st_ = d->stream;
    Stager stage{ws, st_};
    double *dY = stage.up(Y, nC), *dYb = stage.up(Yb, nB), *dRo = stage.up(rhoOld, nC), *dR = stage.up(rho, nC), *dJ = stage.up(phiJmY, nF), *dMu = stage.up(muf, nF);
    double* dSu = Su ? stage.up(Su, nC) : nullptr;
    double *dDf = stage.up(diffusiveFlux, nF), *dNew = stage.scratch(nC);
    uint8_t* dFix = nullptr;
    if (fixedValueFace && nB) {
        dFix = reinterpret_cast<uint8_t*>(stage.scratch((nB + 7) / 8));
        ws.h2d(dFix, fixedValueFace, nB, st_);
    }
    const int rc = qgd_species_step_implicit_dev(d, dY, dYb, dFix, dRo, dR, dJ, dMu, Sc, deltaT, dSu, tolerance, maxIter, dDf, dNew, info);
    if (rc) return rc;
    HIP_CHECK(hipStreamSynchronize(st_));
    ws.d2h(diffusiveFlux, dDf, sizeof(double) * nF, st_);
    ws.d2h(Ynew, dNew, sizeof(double) * nC, st_);
    return QGD_OK;
    QGD_CATCH
}

int qgd_interpolate(qgd_device_t d, int32_t ncomp, const double* cell, const double* bnd, double* out) {
    QGD_TRY
    if (!d || !cell || !out || ncomp < 1 || ncomp > 9 || (!bnd && d->view.nBF > 0)) return fail(QGD_ERR_INVALID, "qgd_interpolate: bad argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    Workspace& ws = d->ws;
    double* dc = ws.get<double>(WS_CELL, (size_t)v.nC * ncomp);
    double* db = ws.get<double>(WS_BND, (size_t)v.nBF * ncomp);
    double* dout = ws.get<double>(WS_OUT, (size_t)v.nF * ncomp);
    ws.h2d(dc, cell, sizeof(double) * (size_t)v.nC * ncomp, d->stream);
    if (v.nBF) ws.h2d(db, bnd, sizeof(double) * (size_t)v.nBF * ncomp, d->stream);
    (void)hipGetLastError();
    launchInterpolate(d->stream, ncomp, v, dc, db, dout);
    HIP_CHECK(hipGetLastError());
    ws.d2h(out, dout, sizeof(double) * (size_t)v.nF * ncomp, d->stream);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
int qgd_flux(qgd_device_t d, int32_t ncomp, const double* flux, const double* psif, double* out) {
    if (!d || !flux || !psif || !out || ncomp < 1) return fail(QGD_ERR_INVALID, "qgd_flux: bad argument");
    const int64_t nF = d->view.nF;
    for (int64_t f = 0; f < nF; ++f)
        for (int k = 0; k < ncomp; ++k) out[f * ncomp + k] = flux[f] * psif[f * ncomp + k];  // flux*psif [QGDInterpolate_8H L104]
    return QGD_OK;
}
int qgd_flux_upwind(qgd_device_t d, int32_t ncomp, const double* flux, const double* cell, const double* bnd, double* out) {
    QGD_TRY
    if (!d || !flux || !cell || !out || ncomp < 1 || ncomp > 9 || (!bnd && d->view.nBF > 0)) return fail(QGD_ERR_INVALID, "qgd_flux_upwind: bad argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    Workspace& ws = d->ws;
    double* dc = ws.get<double>(WS_CELL, (size_t)v.nC * ncomp);
    double* db = ws.get<double>(WS_BND, (size_t)v.nBF * ncomp);
    double* df = ws.get<double>(WS_A, (size_t)v.nF);
    double* dout = ws.get<double>(WS_OUT, (size_t)v.nF * ncomp);
    ws.h2d(dc, cell, sizeof(double) * (size_t)v.nC * ncomp, d->stream);
    if (v.nBF) ws.h2d(db, bnd, sizeof(double) * (size_t)v.nBF * ncomp, d->stream);
    ws.h2d(df, flux, sizeof(double) * (size_t)v.nF, d->stream);
    (void)hipGetLastError();
    launchFluxUpwind(d->stream, ncomp, v, df, dc, db, dout);
    HIP_CHECK(hipGetLastError());
    ws.d2h(out, dout, sizeof(double) * (size_t)v.nF * ncomp, d->stream);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_get(qgd_device_t d, const char* name, double* out, int64_t outDoubles) {
    QGD_TRY
    if (!d || !name || !out) return fail(QGD_ERR_INVALID, "qgd_device_get: null argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& v = d->view;
    const std::string s(name);
    if (s == "hQGDf") {
        if ((int64_t)d->hf.size() > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        std::copy(d->hf.begin(), d->hf.end(), out);
    } else if (s == "hQGD") {
        if (v.nC > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        HIP_CHECK(hipMemcpy(out, v.hQGD, sizeof(double) * (size_t)v.nC, hipMemcpyDeviceToHost));
    } else if (s == "hQGD.boundary") {
        if (v.nBF > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        if (v.nBF) HIP_CHECK(hipMemcpy(out, v.hQGDb, sizeof(double) * (size_t)v.nBF, hipMemcpyDeviceToHost));
    } else return fail(QGD_ERR_UNKNOWN_NAME, "qgd_device_get: unknown name " + s);
    return QGD_OK;
    QGD_CATCH
}

int qgd_poisson_control_default(qgd_poisson_control* c) {
    if (!c) return fail(QGD_ERR_INVALID, "null argument");
    c->tolerance = 1e-6; c->relTol = 0.0; c->maxIter = 1000; c->pRefCell = 0; c->pRefValue = 0.0;
    return QGD_OK;
}

int qgd_qhd_pressure(qgd_device_t d, const double* phiu, const double* phiwo, const double* taubyrhof, const int32_t* patchKind,
                     const double* pb, const double* gradb, const qgd_poisson_control* ctl, double* p, double* phi, double info[3]) {
    QGD_TRY
    if (!d || !phiu || !phiwo || !taubyrhof || !patchKind || !ctl || !p || !phi)
        return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: null argument");
    const MeshView& v = d->view;
    const size_t nC = (size_t)v.nC, nB = (size_t)v.nBF, nF = (size_t)v.nF;
    if (d->sharded()) return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_pressure: the pressure equation is not distributed");
    if (!(ctl->tolerance >= 0) || ctl->maxIter < 0) return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: bad solver controls");
    // per boundary face: 0 nothing to add (zeroGradient, constraint patches), 1 fixedValue, 2 fixedGradient
    std::vector<uint8_t> bKind(std::max<size_t>(nB, 1), 0);
    bool anyFixedValue = false;
    for (size_t ip = 0; ip < d->patches.size(); ++ip) {
        const Patch& pt = d->patches[ip];
        int kind = patchKind[ip];
        if (pt.type != QGD_PATCH_GENERIC) kind = QGD_BC_NONE;  // constraint patches carry no matrix contribution here
        uint8_t k = 0;
        if (kind == QGD_BC_FIXEDVALUE) { k = 1; anyFixedValue = anyFixedValue || pt.size > 0; if (!pb) return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: fixedValue patch without pb"); }
        else if (kind == QGD_BC_QGDFLUX) { k = 2; if (!gradb) return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: fixedGradient patch without gradb"); }
        else if (kind != QGD_BC_ZEROGRADIENT && kind != QGD_BC_NONE) return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: unsupported patch kind");
        for (int32_t f = pt.start; f < pt.start + pt.size; ++f) bKind[(size_t)(f - v.nIF)] = k;
    }
    // fvMatrix::setReference acts only when the field needs a reference level (no fixedValue patch), L0
    int refCell = (!anyFixedValue && ctl->pRefCell >= 0) ? ctl->pRefCell : -1;
    if (refCell >= (int)nC) return fail(QGD_ERR_INVALID, "qgd_qhd_pressure: pRefCell out of range");
    HIP_CHECK(hipSetDevice(d->deviceId));
    DeviceArena tmp;
    try {
        auto upD = [&](const double* src, size_t n) {
            double* dst = tmp.alloc<double>(std::max<size_t>(n, 1), false);
            if (src && n) HIP_CHECK(hipMemcpy(dst, src, sizeof(double) * n, hipMemcpyHostToDevice));
            else { HIP_CHECK(hipMemset(dst, 0, sizeof(double) * std::max<size_t>(n, 1))); HIP_CHECK(hipStreamSynchronize(nullptr)); }
            return dst;
        };
        double* dGamma = upD(taubyrhof, nF);
        double* dPhiu = upD(phiu, nF);
        double* dPhiwo = upD(phiwo, nF);
        double* dPb = upD(pb, nB);
        double* dGb = upD(gradb, nB);
        double* dP = upD(p, nC);
        double* dPhi = tmp.alloc<double>(nF, false);
        uint8_t* dKind = tmp.upload(bKind);
        const size_t nBlocks = (nC + 255) / 256;
        double* work = tmp.alloc<double>(8 * nC + nF + std::max<size_t>(nB, 1) + 3 * nBlocks + 8, false);
        double res[2] = {0, 0};
        (void)hipGetLastError();
        const int iters = solveQhdPressure(d->stream, v, dGamma, dPhiu, dPhiwo, dKind, dPb, dGb, refCell, ctl->pRefValue, ctl->tolerance,
                                           ctl->relTol, ctl->maxIter, dP, dPhi, work, res);
        HIP_CHECK(hipMemcpy(p, dP, sizeof(double) * nC, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(phi, dPhi, sizeof(double) * nF, hipMemcpyDeviceToHost));
        if (info) { info[0] = iters; info[1] = res[0]; info[2] = res[1]; }
    } catch (...) { tmp.release(); throw; }
    tmp.release();
    return QGD_OK;
    QGD_CATCH
}

// ---- case ------------------------------------------------------------------------
int qgd_case_options_default(qgd_case_options* o) {
    if (!o) return fail(QGD_ERR_INVALID, "null argument");
    std::memset(o, 0, sizeof(*o));
    o->stencil = QGD_FVSC_GAUSSVOLPOINT;
    o->implicitDiffusion = 0;
    o->adjustTimeStep = 0;
    o->R = 1.0 / 1.4; o->Cv = (1.0 / 1.4) / 0.4;  // gamma = 1.4, c = 1 at T = 1
    o->mu = 0.0; o->Pr = 1.0;
    o->ScQGD = 1.0; o->PrQGD = 1.0; o->alphaQGD = 0.5;
    o->deltaT = 1e-4; o->maxCo = 0.5; o->maxDeltaT = 1.0; o->cTau = 0.75;
    o->implicitTol = 1e-10; o->implicitMaxIter = 1000;
    return QGD_OK;
}

// ---- what the three creates share -------------------------------------------------------------------------------------------------------
// after an entry's own option checks: the device's refusal of resident cases, the stencil of the options, the device made current
static int caseCreatePreamble(const char* who, qgd_device_s* d, int stencilId, int* st) {
    if (!d->caseRefusal.empty()) return fail(d->caseRefusalCode, std::string(who) + ": " + d->caseRefusal);
    const int rc = deviceStencil(d, stencilId, st);
    if (rc) return rc;
    HIP_CHECK(hipSetDevice(d->deviceId));
    return QGD_OK;
}
static void caseCoreInit(CaseCore* c, qgd_device_s* d, int st) {
    c->dev = d; c->stencil = st;
    c->usesPoints = (st == ST_GVP3 || st == ST_GVP2);
}
// the patch table: every patch zeroGradient or its constraint's own kinds, and the device copy set_fields fills
static void casePatchTable(CaseCore* c) {
    const std::vector<Patch>& patches = c->dev->patches;
    c->bc.resize(patches.size());
    for (size_t i = 0; i < patches.size(); ++i) initPatchBC(c->bc[i], patches[i]);
    c->bcDev = c->arena.alloc<PatchBCDev>(std::max<size_t>(1, c->bc.size()));
}
// the last step of a create: the device counts the case (qgd_device_free refuses while one is open)
static void caseCount(CaseCore* c) {
    c->dev->liveCases++;
    c->counted = true;
}

int qgd_case_create(qgd_device_t d, const qgd_case_options* opt, qgd_case_t* out) {
    QGD_TRY
    if (!d || !opt || !out) return fail(QGD_ERR_INVALID, "qgd_case_create: null argument");
    if (opt->implicitDiffusion && (!(opt->implicitTol >= 0) || opt->implicitMaxIter < 0))
        return fail(QGD_ERR_INVALID, "qgd_case_create: bad implicitTol / implicitMaxIter");
    if (!(opt->R > 0) || !(opt->Cv > 0) || !(opt->Pr > 0) || !(opt->PrQGD > 0) || !(opt->deltaT > 0))
        return fail(QGD_ERR_INVALID, "qgd_case_create: R, Cv, Pr, PrQGD, deltaT must be positive");
    if ((opt->fluxSchemeU != QGD_FLUX_LINEAR && opt->fluxSchemeU != QGD_FLUX_UPWIND) || (opt->fluxSchemeH != QGD_FLUX_LINEAR && opt->fluxSchemeH != QGD_FLUX_UPWIND))
        return fail(QGD_ERR_INVALID, "qgd_case_create: fluxSchemeU / fluxSchemeH must be QGD_FLUX_LINEAR or QGD_FLUX_UPWIND");
    int st = 0;
    const int rc = caseCreatePreamble("qgd_case_create", d, opt->stencil, &st);
    if (rc) return rc;
    qgd_case_s* c = new qgd_case_s();
    try {
        caseCoreInit(c, d, st);
        c->opt = *opt;
        c->pRefresh = c->usesPoints;
        {   // per-term entries [fvsc_8C L51-58]: grad(U), grad(e), grad(rho), grad(p) -> components (Ux,Uy,Uz), e, rho, p of the face gradient
            static const int kBits[4] = {0x0e, 0x20, 0x01, 0x10};
            int term[4], lo = st, hi = st;
            for (int t = 0; t < 4; ++t) {
                term[t] = st;
                if (opt->termStencil[t] != 0) {
                    const int r2 = deviceStencil(d, opt->termStencil[t] - 1, &term[t]);   // the checks of fvscOpName apply per term
                    if (r2) return caseAbandon(c, r2);
                }
                lo = std::min(lo, term[t]); hi = std::max(hi, term[t]);
            }
            for (int t = 0; t < 4; ++t)
                if (term[t] != lo && term[t] != hi)
                    return caseAbandon(c, fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_create: more than two distinct fvsc stencils in one case"));
            if (lo != hi) {
                c->stencil = lo; c->mixB = hi; c->mixMask = 0;
                for (int t = 0; t < 4; ++t) if (term[t] == hi) c->mixMask |= kBits[t];
                c->usesPoints = (hi == ST_GVP3 || hi == ST_GVP2 || lo == ST_GVP3 || lo == ST_GVP2);
            } else c->stencil = lo;
            c->pRefresh = (term[3] == ST_GVP3 || term[3] == ST_GVP2);
        }
        GasModel& g = c->gas;
        g.R = opt->R; g.Cv = opt->Cv; g.mu0 = opt->mu; g.Pr = opt->Pr; g.ScQGD = opt->ScQGD; g.PrQGD = opt->PrQGD; g.rPrQGD = 1.0 / opt->PrQGD;
        g.alphaQGD = opt->alphaQGD;
        g.consistentEnergy = opt->consistentEnergy ? 1 : 0;
        g.implicitDiffusion = opt->implicitDiffusion ? 1 : 0;
        g.upwindU = opt->fluxSchemeU == QGD_FLUX_UPWIND ? 1 : 0;
        g.upwindH = opt->fluxSchemeH == QGD_FLUX_UPWIND ? 1 : 0;
        const double Cp = opt->Cv + opt->R;
        g.gamma = Cp / opt->Cv;
        const double rPr = 1.0 / opt->Pr;
        g.alphah0 = (Cp * opt->mu * rPr) / Cp;
        const MeshView& v = d->view;
        DeviceArena& a = c->arena;
        CaseView& cv = c->view;
        cv.A = a.alloc<RecA>(v.nC); cv.B = a.alloc<RecB>(v.nC); cv.rE = a.alloc<double>(v.nC);
        cv.P = a.alloc<RecA>(v.nP);
        // the fused step (fusedFaceCellKernel): uniform 3-D GaussVolPoint, explicit, fixed deltaT; `Gauss upwind` fluxes are an instantiation
        c->fused = v.fuBlocks > 0 && c->stencil == ST_GVP3 && c->mixB < 0 && !opt->implicitDiffusion && !opt->adjustTimeStep;
        if (c->fused) { cv.A2 = a.alloc<RecA>(v.nC); cv.B2 = a.alloc<RecB>(v.nC); }
        {   // the same blocks under Courant-number control: two launches (blocks up to their sums, then the cells) instead of three kernels
            c->fusedAdj = v.fuBlocks > 0 && c->stencil == ST_GVP3 && c->mixB < 0 && !opt->implicitDiffusion && opt->adjustTimeStep &&
                          envOnOff("QGD_FUSED_ADJUST", 1) != 0;
            if (c->fusedAdj) cv.cellSum = a.alloc<double>(5 * (size_t)v.nC);
        }
        // the reference's default branch on the same blocks (unsharded, fixed deltaT, one 3-D GaussVolPoint stencil)
        c->fusedImpl = v.fuBlocks > 0 && v.fuLdsImpl > 0 && c->stencil == ST_GVP3 && c->mixB < 0 && opt->implicitDiffusion && !opt->adjustTimeStep &&
                       !d->sharded() && envOnOff("QGD_IMPL_FUSED", 1) != 0 && fusedImplUPrepare(v, c->gas);
        cv.bA = a.alloc<RecA>(v.nBF); cv.bB = a.alloc<RecB>(v.nBF);
        cv.bG = a.alloc<double>(v.nBF); cv.bPhiw = a.alloc<double>(v.nBF); cv.bPmid = a.alloc<double>(v.nBF);
        cv.bRhoLag = a.alloc<double>(v.nBF);
        // (the cell blocks under Courant-number control get slots of their own behind the patch kernel's: a mesh of small blocks has more
        // blocks than 64-face tiles, and a block that wrote into the tiles' slots would overwrite the patch faces' partials and run past the table)
        cv.fuBlkFace = faceBlocks(v) + bfaceBlocks(v);
        cv.nBlkFace = cv.fuBlkFace + (c->fusedAdj ? v.fuBlocks : 0);
        cv.nBlkCell = std::max(cellBlocks(v), v.fuBlocks) + (d->nSendAll + 63) / 64;   // (the fused kernel monitors min(rho), min(e) per block)
        cv.blkFace = a.alloc<double>(2 * (size_t)std::max(1, cv.nBlkFace));
        cv.blkFace2 = a.alloc<double>(2 * (size_t)QGD_FACE_REDUCE_PARTIALS);
        cv.blkCell = a.alloc<double>(2 * (size_t)std::max(1, cv.nBlkCell));
        cv.flux = a.alloc<double>(5 * (size_t)v.nF);
        cv.red = a.alloc<double>(8);
        cv.dt = a.alloc<double>(8);
        cv.dbg = nullptr;
        if (opt->implicitDiffusion) {
            ImplView& iv = c->impl;
            const size_t nC = (size_t)v.nC, nF = (size_t)v.nF;
            d->ensureFaceGeoPos();
            iv.gUc = a.alloc<double>(9 * nC);
            iv.phiTau = a.alloc<double>(3 * nF); iv.UfS = a.alloc<double>(3 * nF);
            iv.sTau = a.alloc<double>(nF); iv.mufS = a.alloc<double>(nF); iv.aU = a.alloc<double>(nF); iv.aE = a.alloc<double>(nF);
            iv.phiSig = a.alloc<double>(nF);
            iv.rhoNew = a.alloc<double>(nC);
            iv.xU = a.alloc<double>(3 * nC); iv.diagU = a.alloc<double>(3 * nC); iv.rhsU = a.alloc<double>(3 * nC);
            iv.xE = a.alloc<double>(nC); iv.diagE = a.alloc<double>(nC); iv.rhsE = a.alloc<double>(nC);
            c->implSolver = implicitSolverCreate(d->stream, v, d->ownedBegin, d->ownedEnd);
            c->reuseGradU = envOnOff("QGD_IMPL_REUSE_GRADU", 1) != 0;
            {   // start values of the two solves (qgd_implicit.hip "start values"): 0 = OpenFOAM's (the predictor), 1..3 = + the extrapolated correction
                static const int kOrders[] = {0, 1, 2, 3, 4};
                c->implXOrder = envChoice("QGD_IMPL_XEXTRAP", 3, kOrders, 5);
                if (c->implXOrder > 0) {
                    iv.pred = a.alloc<double>(4 * nC);
                    for (int j = 0; j < c->implXOrder; ++j) iv.dh[j] = a.alloc<double>(4 * nC);
                }
                iv.have = 0; iv.order = c->implXOrder;
                iv.w = nullptr; iv.dtHist = nullptr;
                if (c->implXOrder > 0 && opt->adjustTimeStep) { iv.w = a.alloc<double>(4); iv.dtHist = a.alloc<double>(8); }   // (zero-filled)
            }
        }
        casePatchTable(c);
        const double dt0[8] = {opt->deltaT, 0, 0, 0, 0, 0, 0, 0};
        HIP_CHECK(hipMemcpy(cv.dt, dt0, sizeof(dt0), hipMemcpyHostToDevice));
    } catch (...) { caseAbandon(c, 0); throw; }
    caseCount(c);
    *out = c;
    return QGD_OK;
    QGD_CATCH
}
int qgd_case_free(qgd_case_t c) {
    if (!c) return QGD_OK;
    (void)hipSetDevice(c->dev->deviceId);
    harvestTiming(c);
    for (hipEvent_t e : c->freeEvents) (void)hipEventDestroy(e);
    if (c->ownHaloStream) { (void)hipStreamSynchronize(c->ownHaloStream); (void)hipStreamDestroy(c->ownHaloStream); }
    if (c->evLayerDone) (void)hipEventDestroy(c->evLayerDone);
    if (c->evUnpacked) (void)hipEventDestroy(c->evUnpacked);
    return caseAbandon(c, QGD_OK);
}

// CaseView::bValU / bValT / bValP follow the patches' flags: a field no patch has a list for reads nothing (nullptr)
static void bcValuePointers(qgd_case_s* c) {
    int32_t any = 0;
    for (const PatchBCDev& b : c->bc) any |= b.valList;
    c->view.bValU = (any & QGD_BC_LIST_U) ? c->bcValDev[0] : nullptr;
    c->view.bValT = (any & QGD_BC_LIST_T) ? c->bcValDev[1] : nullptr;
    c->view.bValP = (any & QGD_BC_LIST_P) ? c->bcValDev[2] : nullptr;
}
// the block-fused assembly of the U systems reads a fixedValue patch's one velocity out of the table (implCellU inside
// fusedFaceCellKernel<..., IMPL>): a case with per-face velocities assembles with implCellUKernel, which reads the list
static bool implFusedNow(const qgd_case_s* c) { return c->fusedImpl && !c->view.bValU; }

// The write of one patch's table entry behind the three set_bc: `who` names the entry.  pKinds: the p kinds the case admits on top of
// zeroGradient / fixedValue / none -- 0: a case without p (its entry keeps zeroGradient, or the constraint's kind), 1: qgdFlux, 2: and qhdFlux
static int casePatchEntry(CaseCore* c, const char* who, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT, int pKinds,
                          int32_t bcP, double valueP) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    const std::string w(who);
    if (patch < 0 || patch >= (int32_t)c->bc.size()) return fail(QGD_ERR_INVALID, w + ": patch out of range");
    auto okU = [](int k) { return k == QGD_BC_ZEROGRADIENT || k == QGD_BC_FIXEDVALUE || k == QGD_BC_SLIP || k == QGD_BC_NONE; };
    auto okT = [](int k) { return k == QGD_BC_ZEROGRADIENT || k == QGD_BC_FIXEDVALUE || k == QGD_BC_NONE; };
    auto okP = [pKinds](int k) {
        return k == QGD_BC_ZEROGRADIENT || k == QGD_BC_FIXEDVALUE || k == QGD_BC_NONE || (pKinds >= 1 && k == QGD_BC_QGDFLUX) || (pKinds >= 2 && k == QGD_BC_QHDFLUX);
    };
    if (!okU(bcU) || !okT(bcT) || !okP(bcP)) return fail(QGD_ERR_INVALID, w + ": unsupported boundary-condition kind");
    PatchBCDev& b = c->bc[patch];
    constraintKinds(b.ptype, bcU, bcT, bcP);   // a constraint patch keeps its own field type whatever the caller asks for
    b.bcU = bcU; b.bcT = bcT; b.bcP = bcP; b.vT = valueT; b.vP = valueP;
    if (valueU) for (int k = 0; k < 3; ++k) b.vU[k] = valueU[k];
    b.valList = 0;   // the patch is uniform again: a value list follows its entry (*_set_bc_values comes after this call)
    c->fieldsSet = false;
    return QGD_OK;
}
int qgd_case_set_bc(qgd_case_t c, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT, int32_t bcP, double valueP) {
    QGD_TRY
    const int rc = casePatchEntry(c, "qgd_case_set_bc", patch, bcU, valueU, bcT, valueT, 1, bcP, valueP);
    if (rc) return rc;
    bcValuePointers(c);
    c->gradUValid = false;
    return QGD_OK;
    QGD_CATCH
}

// field 0 U, 1 T, 2 p of a patch's table entry
static int32_t bcKindOf(const PatchBCDev& b, int field) { return field == 0 ? b.bcU : (field == 1 ? b.bcT : b.bcP); }
// The checks of a per-face value list of a fixedValue entry (both set_bc_values, qgd_case_get_bc_values).  counted: nFaces has to be the
// patch's (a null list, which clears the flag, comes with any).  noEntry: the one text an entry has for a halo, cyclic or constraint patch
// (behind the patch's name), nullptr: one text per kind of patch.
static int bcValuesCheck(CaseCore* c, const char* who, int32_t patch, int32_t field, int64_t nFaces, bool counted, const char* noEntry = nullptr) {
    const std::string w(who);
    if (!c) return fail(QGD_ERR_INVALID, w + ": null case");
    if (patch < 0 || patch >= (int32_t)c->bc.size()) return fail(QGD_ERR_INVALID, w + ": patch out of range");
    if (field < 0 || field > 2) return fail(QGD_ERR_INVALID, w + ": field must be 0 (U), 1 (T) or 2 (p)");
    const Patch& pt = c->dev->patches[patch];
    const PatchBCDev& b = c->bc[patch];
    static const char* kFieldName[3] = {"U", "T", "p"};
    if (pt.type != QGD_PATCH_GENERIC && noEntry) return fail(QGD_ERR_INVALID, w + ": patch '" + pt.name + noEntry);
    if (pt.type == QGD_PATCH_HALO) return fail(QGD_ERR_INVALID, w + ": patch '" + pt.name + "' is a halo patch (its faces carry no boundary condition)");
    if (pt.type == QGD_PATCH_CYCLIC) return fail(QGD_ERR_INVALID, w + ": patch '" + pt.name + "' is a cyclic patch (its faces carry no boundary condition)");
    if (pt.type != QGD_PATCH_GENERIC)
        return fail(QGD_ERR_INVALID, w + ": patch '" + pt.name + "' is a constraint patch (empty / symmetryPlane / symmetry / wedge): it keeps its own field type");
    if (bcKindOf(b, field) != QGD_BC_FIXEDVALUE)
        return fail(QGD_ERR_INVALID, w + ": the " + kFieldName[field] + " entry of patch '" + pt.name + "' is not fixedValue (per-face values belong to fixedValue entries only)");
    if (counted && nFaces != (int64_t)pt.size)
        return fail(QGD_ERR_INVALID, w + ": patch '" + pt.name + "' has " + std::to_string(pt.size) + " faces on this device's mesh, nFaces = " + std::to_string(nFaces));
    return QGD_OK;
}
// The store behind both set_bc_values, after the check: the list of `field` (3 per face for U, else 1) goes into devList, one entry per
// boundary face of the device's mesh and made on first use, and into hostList where the case keeps a host copy; a null list clears the
// patch's flag.  finite: a non-finite value is refused.  The caller refreshes its view's pointers.
static int bcValuesStore(CaseCore* c, const char* who, int32_t patch, int32_t field, const double* values, bool finite, double*& devList,
                         std::vector<double>* hostList) {
    const std::string w(who);
    const Patch& pt = c->dev->patches[patch];
    const int32_t bit = 1 << field;
    if (!values) c->bc[patch].valList &= ~bit;
    else {
        HIP_CHECK(hipSetDevice(c->dev->deviceId));
        const MeshView& m = c->dev->view;
        const size_t nw = field == 0 ? 3 : 1, nB = (size_t)m.nBF, first = (size_t)(pt.start - m.nIF);
        if (first + (size_t)pt.size > nB) return fail(QGD_ERR_INVALID, w + ": the patch's faces lie outside the device's boundary faces");
        if (finite)
            for (size_t i = 0; i < nw * (size_t)pt.size; ++i)
                if (!std::isfinite(values[i])) return fail(QGD_ERR_INVALID, w + ": non-finite value");
        if (hostList && hostList->empty()) hostList->assign(nw * std::max<size_t>(nB, 1), 0.0);
        if (!devList) devList = c->arena.alloc<double>(nw * std::max<size_t>(nB, 1));   // (zero-filled)
        if (pt.size > 0) {
            if (hostList) std::memcpy(hostList->data() + nw * first, values, sizeof(double) * nw * (size_t)pt.size);
            HIP_CHECK(hipStreamSynchronize(c->stream()));   // (no kernel of an earlier step still reads the old values)
            HIP_CHECK(hipMemcpy(devList + nw * first, values, sizeof(double) * nw * (size_t)pt.size, hipMemcpyHostToDevice));
        }
        c->bc[patch].valList |= bit;
    }
    c->fieldsSet = false;   // like set_bc: the patch records are evaluated again by set_fields
    return QGD_OK;
}

int qgd_case_set_bc_values(qgd_case_t c, int32_t patch, int32_t field, const double* values, int64_t nFaces) {
    QGD_TRY
    int rc = bcValuesCheck(c, "qgd_case_set_bc_values", patch, field, nFaces, values != nullptr);
    if (rc == QGD_OK) rc = bcValuesStore(c, "qgd_case_set_bc_values", patch, field, values, false, c->bcValDev[field], &c->bcValHost[field]);
    if (rc) return rc;
    bcValuePointers(c);
    c->ghostsCurrent = false;  // the copies behind cyclic halves take their originals' records after qgd_case_set_fields
    c->gradUValid = false;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_get_bc_values(qgd_case_t c, int32_t patch, int32_t field, double* values, int64_t nFaces, int32_t* isList) {
    QGD_TRY
    const int rc = bcValuesCheck(c, "qgd_case_get_bc_values", patch, field, nFaces, true);
    if (rc) return rc;
    if (!values && nFaces > 0) return fail(QGD_ERR_INVALID, "qgd_case_get_bc_values: null argument");
    const MeshView& m = c->dev->view;
    const Patch& pt = c->dev->patches[patch];
    const PatchBCDev& b = c->bc[patch];
    const bool list = (b.valList & (1 << field)) != 0;
    const size_t w = field == 0 ? 3 : 1, first = (size_t)(pt.start - m.nIF);
    if (list) std::memcpy(values, c->bcValHost[field].data() + w * first, sizeof(double) * w * (size_t)pt.size);
    else
        for (int64_t i = 0; i < nFaces; ++i) {
            if (field == 0) for (int k = 0; k < 3; ++k) values[3 * i + k] = b.vU[k];
            else values[i] = field == 1 ? b.vT : b.vP;
        }
    if (isList) *isList = list ? 1 : 0;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_set_qgd_coeffs(qgd_case_t c, const double* alphaQGD, const double* alphaQGDb, const double* ScQGD, const double* ScQGDb) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (c->dev->view.nBF > 0 && ((alphaQGD && !alphaQGDb) || (ScQGD && !ScQGDb)))
        return fail(QGD_ERR_INVALID, "qgd_case_set_qgd_coeffs: a field needs both its cell and its patch values");
    if (c->varSc && ScQGD)
        return fail(QGD_ERR_INVALID, "qgd_case_set_qgd_coeffs: the case runs varScModel7 (qgd_case_set_var_sc), which computes ScQGD itself; "
                                     "pass ScQGD = NULL, or drop the model first");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MeshView& m = c->dev->view;
    auto put = [&](const double* src, size_t n, double*& slot) -> const double* {
        if (!src) return nullptr;
        if (!slot) slot = c->arena.alloc<double>(std::max<size_t>(n, 1), false);
        if (n) HIP_CHECK(hipMemcpy(slot, src, sizeof(double) * n, hipMemcpyHostToDevice));
        return slot;
    };
    c->view.aQ = put(alphaQGD, (size_t)m.nC, c->coef[0]);
    c->view.aQb = put(alphaQGD ? alphaQGDb : nullptr, (size_t)m.nBF, c->coef[1]);
    if (!c->varSc) {
        c->view.sc = put(ScQGD, (size_t)m.nC, c->coef[2]);
        c->view.scb = put(ScQGD ? ScQGDb : nullptr, (size_t)m.nBF, c->coef[3]);
    }
    c->fieldsSet = false;
    c->gradUValid = false;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_set_var_sc(qgd_case_t c, const qgd_var_sc_options* opt, const int32_t* constCells) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    qgd_device_s* d = c->dev;
    const MeshView& m = d->view;
    if (!opt) {
        if (c->varSc) { c->varSc = false; c->view.sc = nullptr; c->view.scb = nullptr; c->fieldsSet = false; c->gradUValid = false; }
        return QGD_OK;
    }
    if (opt->model != 7)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_var_sc: model " + std::to_string(opt->model) + " is not served (varScModel7 only: model = 7)");
    if (d->periodic())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_var_sc: varScModel7 is not served on a periodic device (cyclic patches served by ghost copies, "
                                             "qgd_mesh_unroll_cyclic): such a case runs with uniform coefficients");
    if (!c->varSc && c->view.sc)
        return fail(QGD_ERR_INVALID, "qgd_case_set_var_sc: the case carries a ScQGD array (qgd_case_set_qgd_coeffs); varScModel7 computes ScQGD itself -- "
                                     "drop the array first (alphaQGD arrays may stay)");
    if (!std::isfinite(opt->ScQGD) || !std::isfinite(opt->cSc1) || !std::isfinite(opt->minSc) || !std::isfinite(opt->maxSc))
        return fail(QGD_ERR_INVALID, "qgd_case_set_var_sc: ScQGD, cSc1, minSc, maxSc must be finite");
    if (opt->nConstCells < 0 || (opt->nConstCells > 0 && !constCells))
        return fail(QGD_ERR_INVALID, "qgd_case_set_var_sc: nConstCells cells need their labels");
    for (int32_t i = 0; i < opt->nConstCells; ++i)
        if (constCells[i] < 0 || constCells[i] >= m.nC)
            return fail(QGD_ERR_INVALID, "qgd_case_set_var_sc: cell label " + std::to_string(constCells[i]) + " of constCells is out of range [0, " +
                                         std::to_string(m.nC) + ")");
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    VarScView v{};
    v.rf = d->ensureSensorRatio();
    if (!c->coef[2]) c->coef[2] = c->arena.alloc<double>(std::max<size_t>((size_t)m.nC, 1), false);
    if (!c->coef[3]) c->coef[3] = c->arena.alloc<double>(std::max<size_t>((size_t)m.nBF, 1), false);
    if (!c->scPart) c->scPart = c->arena.alloc<double>(2 * (size_t)QGD_FACE_REDUCE_PARTIALS + 2);
    // the constructor's field: the dictionary value everywhere [L77-84]; patch values keep it, clipped like the field [L237-244]
    double scb = opt->ScQGD;
    if (opt->minSc >= 0.0) scb = std::max(scb, opt->minSc);
    if (opt->maxSc >= 0.0) scb = std::min(scb, opt->maxSc);
    {
        const std::vector<double> fillC((size_t)m.nC, opt->ScQGD), fillB((size_t)m.nBF, scb);
        if (m.nC) HIP_CHECK(hipMemcpy(c->coef[2], fillC.data(), sizeof(double) * fillC.size(), hipMemcpyHostToDevice));
        if (m.nBF) HIP_CHECK(hipMemcpy(c->coef[3], fillB.data(), sizeof(double) * fillB.size(), hipMemcpyHostToDevice));
    }
    v.constCell = nullptr;
    if (opt->nConstCells > 0) {
        std::vector<uint8_t> mask((size_t)m.nC, 0);
        for (int32_t i = 0; i < opt->nConstCells; ++i) mask[(size_t)constCells[i]] = 1;
        if (!c->constCellDev) c->constCellDev = c->arena.alloc<uint8_t>((size_t)m.nC, false);
        HIP_CHECK(hipMemcpy(c->constCellDev, mask.data(), mask.size(), hipMemcpyHostToDevice));
        v.constCell = c->constCellDev;
    }
    v.sc = c->coef[2]; v.part = c->scPart;
    v.ScQGD = opt->ScQGD; v.cSc1 = opt->cSc1; v.minSc = opt->minSc; v.maxSc = opt->maxSc;
    c->vsc = v;
    c->view.sc = c->coef[2];
    c->view.scb = c->coef[3];
    c->varSc = true;
    c->fieldsSet = false;
    c->gradUValid = false;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_sc_range(qgd_case_t c, double out[2]) {
    QGD_TRY
    if (!c || !out) return fail(QGD_ERR_INVALID, "null argument");
    const qgd_device_s* d = c->dev;
    if (!c->view.sc || d->ownedEnd <= d->ownedBegin) { out[0] = out[1] = c->gas.ScQGD; return QGD_OK; }
    HIP_CHECK(hipSetDevice(d->deviceId));
    if (!c->scPart) c->scPart = c->arena.alloc<double>(2 * (size_t)QGD_FACE_REDUCE_PARTIALS + 2);
    VarScView v = c->vsc;
    v.sc = const_cast<double*>(c->view.sc); v.part = c->scPart;
    (void)hipGetLastError();
    launchVarScRange(c->stream(), v, d->ownedBegin, d->ownedEnd);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, c->scPart + 2 * (size_t)QGD_FACE_REDUCE_PARTIALS, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream()));
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    return QGD_OK;
    QGD_CATCH
}

// ---- species mass fractions carried by the case (qgd_species.hip) ---------------------------------------------------------------
int qgd_case_set_species(qgd_case_t c, int32_t nSpecies, int32_t inertIndex, const double* ScNumbers, int32_t flags) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    qgd_device_s* d = c->dev;
    if (c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_set_species: call it before qgd_case_set_fields");
    if (c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species: the case carries species already");
    if (c->opt.implicitDiffusion && !(flags & QGD_SPECIES_IMPLICIT))
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_species: implicitDiffusion true is not served without the flag QGD_SPECIES_IMPLICIT (the species equations' "
                                             "fvm::laplacian branch, QGDYEqn.H L47-66, solves one linear system per batch of species inside the step: a caller asks for it by "
                                             "name); pass the flag, or set implicitDiffusion false");
    const bool halo = (flags & QGD_SPECIES_HALO) != 0;   // the state message carries the composition (asked for by name)
    if (d->periodic() && !halo)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_species: a periodic device (cyclic patches served by ghost copies, qgd_mesh_unroll_cyclic) is not served: "
                                             "the copies would need the species' values");
    if (d->sharded() && !halo)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_species: a sharded device is not served (the halo messages carry no species)");
    if (d->sharded() && c->opt.implicitDiffusion)   // (a periodic device is sharded() too)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_species: implicitDiffusion true with species on a sharded or periodic device is not served: the batched "
                                             "species solves are not distributed (no messages, no reductions across ghosts); use the explicit branch");
    if (c->mixB >= 0)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_set_species: per-term stencils (qgd_case_options::termStencil) are not served: fvsc::grad(Y) has no entry of its own");
    if (nSpecies < 2) return fail(QGD_ERR_INVALID, "qgd_case_set_species: nSpecies must be at least 2 (one transported species and the inert one)");
    if (nSpecies > QGD_MAX_SPECIES) return fail(QGD_ERR_INVALID, "qgd_case_set_species: at most " + std::to_string(QGD_MAX_SPECIES) + " species are served");
    if (inertIndex < 0 || inertIndex >= nSpecies) return fail(QGD_ERR_INVALID, "qgd_case_set_species: inertIndex out of range");
    if (flags & ~(QGD_SPECIES_KEEP_FLUXES | QGD_SPECIES_IMPLICIT | QGD_SPECIES_HALO)) return fail(QGD_ERR_INVALID, "qgd_case_set_species: unknown flags");
    for (int32_t i = 0; ScNumbers && i < nSpecies; ++i)
        if (!(ScNumbers[i] > 0) || !std::isfinite(ScNumbers[i]))
            return fail(QGD_ERR_INVALID, "qgd_case_set_species: the Schmidt number of species " + std::to_string(i) + " must be positive (Sc <= 0)");
    static_assert(QGD_MAX_SPECIES <= QGD_MAX_SPECIES_DEV, "SpeciesView tables");
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& m = d->view;
    DeviceArena& a = c->arena;
    SpeciesView sv{};
    const size_t nS = (size_t)nSpecies, nP = std::max<size_t>(c->bc.size(), 1);
    sv.nS = nSpecies; sv.inert = inertIndex; sv.nPatches = (int32_t)nP;
    for (int32_t i = 0; i < nSpecies; ++i) {
        sv.Sc[i] = ScNumbers ? ScNumbers[i] : 1.0;
        if (i != inertIndex) sv.act[sv.nAct++] = i;
    }
    sv.Y = a.alloc<double>(nS * std::max<size_t>((size_t)m.nC, 1));
    sv.Yb = a.alloc<double>(nS * std::max<size_t>((size_t)m.nBF, 1));
    const size_t nAct = (size_t)sv.nAct;   // the inert species is not transported: no vertex values, no face flux of its own
    sv.ptY = c->usesPoints ? a.alloc<double>(nAct * std::max<size_t>((size_t)m.nP, 1)) : nullptr;
    sv.F = a.alloc<double>(nAct * std::max<size_t>((size_t)m.nF, 1));
    c->spKeep = (flags & QGD_SPECIES_KEEP_FLUXES) != 0;
    if (c->spKeep) { sv.phiJmY = a.alloc<double>(nS * std::max<size_t>((size_t)m.nF, 1)); sv.dflux = a.alloc<double>(nS * std::max<size_t>((size_t)m.nF, 1)); }
    c->spBcKindDev = a.alloc<uint8_t>(nS * nP);
    c->spBcValDev = a.alloc<double>(nS * nP);
    sv.bcKind = c->spBcKindDev; sv.bcVal = c->spBcValDev;
    c->spBcKind.assign(nS * nP, (uint8_t)QGD_BC_NONE);
    c->spBcVal.assign(nS * nP, 0.0);
    for (size_t i = 0; i < nS; ++i)
        for (size_t p = 0; p < c->bc.size(); ++p)
            if (d->patches[p].type == QGD_PATCH_GENERIC) c->spBcKind[i * nP + p] = (uint8_t)QGD_BC_ZEROGRADIENT;
    c->spFieldSet.assign(nS, 0);
    if (c->opt.implicitDiffusion) {   // [QGDYEqn.H L47-66]: one solve per register batch
        const size_t cells = std::max<size_t>((size_t)m.nC, 1);
        c->spImpl.aF = a.alloc<double>(std::max<size_t>((size_t)m.nF, 1));
        c->spImpl.diag = a.alloc<double>(4 * cells);
        c->spImpl.rhs = a.alloc<double>(4 * cells);
        c->spImpl.x = a.alloc<double>((nAct + 3) * cells);
        c->spBatches = (sv.nAct + speciesBatchWidth() - 1) / speciesBatchWidth();
        const size_t nStat = (size_t)implicitStatsDoubles(c->spBatches);
        c->spStats = a.alloc<double>(nStat);
        HIP_CHECK(hipMemset(c->spStats, 0, sizeof(double) * nStat));
    }
    c->sp = sv;
    c->spDirty = true;
    c->spFluxesValid = false;
    c->spHalo = halo;
    if (halo) { c->haloBuf.send.clear(); c->haloBuf.recv.clear(); }   // (the case's own message buffers are sized for the wider state message on their next use)
    // the species block reads phiJm of every face, which the fused kernels never write: the three-kernel explicit step, or the separate
    // kernels of the implicit branch (the block-fused assembly of the U systems keeps the internal faces' mass flux in its blocks)
    c->fused = false;
    c->fusedAdj = false;
    c->fusedImpl = false;
    c->view.nBlkFace = c->view.fuBlkFace;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_set_species_bc(qgd_case_t c, int32_t species, int32_t patch, int32_t bc, double value) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species_bc: the case carries no species (qgd_case_set_species)");
    if (species < 0 || species >= c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species_bc: species out of range");
    if (patch < 0 || patch >= (int32_t)c->bc.size()) return fail(QGD_ERR_INVALID, "qgd_case_set_species_bc: patch out of range");
    if (bc != QGD_BC_ZEROGRADIENT && bc != QGD_BC_FIXEDVALUE && bc != QGD_BC_NONE)
        return fail(QGD_ERR_INVALID, "qgd_case_set_species_bc: a species takes zeroGradient, fixedValue or none");
    if (bc == QGD_BC_FIXEDVALUE && !std::isfinite(value)) return fail(QGD_ERR_INVALID, "qgd_case_set_species_bc: the value must be finite");
    if (c->dev->patches[patch].type != QGD_PATCH_GENERIC) bc = QGD_BC_NONE;   // a constraint patch keeps its own field type
    const size_t e = (size_t)species * c->sp.nPatches + patch;
    c->spBcKind[e] = (uint8_t)bc;
    c->spBcVal[e] = bc == QGD_BC_FIXEDVALUE ? value : 0.0;
    c->spDirty = true;
    c->ghostsCurrent = false;   // (a periodic device: the copies' patch values follow the new rule with the next refresh)
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_set_species_fields(qgd_case_t c, int32_t species, const double* Y) {
    QGD_TRY
    if (!c || !Y) return fail(QGD_ERR_INVALID, "qgd_case_set_species_fields: null argument");
    if (!c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species_fields: the case carries no species (qgd_case_set_species)");
    if (species < 0 || species >= c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species_fields: species out of range");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MeshView& m = c->dev->view;
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    if (m.nC) HIP_CHECK(hipMemcpy(c->sp.Y + (size_t)species * m.nC, Y, sizeof(double) * (size_t)m.nC, hipMemcpyHostToDevice));
    c->spFieldSet[species] = 1;
    c->spDirty = true;
    c->spFluxesValid = false;
    c->ghostsCurrent = false;   // (a periodic device: the copies take their originals' composition before the first step)
    return QGD_OK;
    QGD_CATCH
}

// before the first use after a change: every species has its field, the boundary-condition tables are on the device, the patch values follow them
static int speciesReady(qgd_case_s* c, const char* who) {
    for (int32_t i = 0; i < c->sp.nS; ++i)
        if (!c->spFieldSet[i])
            return fail(QGD_ERR_INVALID, std::string(who) + ": the field of species " + std::to_string(i) + " was never set (qgd_case_set_species_fields)");
    if (!c->spDirty) return QGD_OK;
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    HIP_CHECK(hipMemcpy(c->spBcKindDev, c->spBcKind.data(), c->spBcKind.size(), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(c->spBcValDev, c->spBcVal.data(), sizeof(double) * c->spBcVal.size(), hipMemcpyHostToDevice));
    (void)hipGetLastError();
    launchSpeciesPatchValues(c->stream(), c->dev->view, c->sp, -1);   // every face, those of ghost cells too, from the values the caller set
    HIP_CHECK(hipGetLastError());
    c->spDirty = false;
    return QGD_OK;
}

int qgd_case_get_species_field(qgd_case_t c, int32_t species, const char* name, double* out, int64_t outDoubles) {
    QGD_TRY
    if (!c || !name || !out) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: null argument");
    if (!c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: the case carries no species (qgd_case_set_species)");
    if (species < 0 || species >= c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: species out of range");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MeshView& m = c->dev->view;
    const std::string s(name);
    const double* src = nullptr;
    int64_t n = 0;
    if (s == "Y" || s == "Y.boundary") {
        if (!c->spFieldSet[species]) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: the field of species " + std::to_string(species) + " was never set");
        if (s == "Y") { src = c->sp.Y + (size_t)species * m.nC; n = m.nC; }
        else {
            const int rs = speciesReady(c, "qgd_case_get_species_field");
            if (rs) return rs;
            src = c->sp.Yb + (size_t)species * m.nBF; n = m.nBF;
        }
    } else if (s == "phiJmY" || s == "diffusiveFlux") {
        if (!c->spKeep) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: " + s + " is kept with QGD_SPECIES_KEEP_FLUXES only");
        if (!c->spFluxesValid) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: " + s + " is formed by a step; none has run since the fields were set");
        src = (s == "phiJmY" ? c->sp.phiJmY : c->sp.dflux) + (size_t)species * m.nF; n = m.nF;
    } else return fail(QGD_ERR_UNKNOWN_NAME, "qgd_case_get_species_field: unknown field " + s);
    if (n > outDoubles) return fail(QGD_ERR_INVALID, "qgd_case_get_species_field: output too small");
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    if (n) HIP_CHECK(hipMemcpy(out, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_set_species_solver(qgd_case_t c, double tolerance, int32_t maxIter) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_case_set_species_solver: the case carries no species (qgd_case_set_species)");
    if (!c->opt.implicitDiffusion) return fail(QGD_ERR_INVALID, "qgd_case_set_species_solver: the explicit branch of the species equations solves nothing (implicitDiffusion false)");
    if (!(tolerance > 0) || !std::isfinite(tolerance) || maxIter < 1)
        return fail(QGD_ERR_INVALID, "qgd_case_set_species_solver: tolerance must be positive, maxIter >= 1");
    c->spTol = tolerance;
    c->spMaxIter = maxIter;
    return QGD_OK;
}
int qgd_case_species_implicit_info(qgd_case_t c, double* info, int64_t infoDoubles) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    if (!c->sp.nS || !c->spStats || !c->implSolver)
        return fail(QGD_ERR_INVALID, "qgd_case_species_implicit_info: a case with species on the implicitDiffusion branch (qgd_case_set_species)");
    const int64_t need = 3 + 3 * (int64_t)c->sp.nS;
    if (infoDoubles < need) return fail(QGD_ERR_INVALID, "qgd_case_species_implicit_info: output too small (3 + 3 nSpecies doubles)");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    implicitSolverSetStream(c->implSolver, c->stream());
    for (int64_t k = 0; k < need; ++k) info[k] = 0.0;
    std::vector<double> act(3 * (size_t)c->sp.nAct);
    implicitStatsRead(c->implSolver, c->spStats, c->spBatches, speciesBatchWidth(), c->sp.nAct, act.data(), &info[0], &info[1]);
    info[2] = c->sp.nS;
    for (int a = 0; a < c->sp.nAct; ++a)
        for (int j = 0; j < 3; ++j) info[3 + 3 * c->sp.act[a] + j] = act[3 * (size_t)a + j];
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_species_info(qgd_case_t c, int64_t info[4]) {
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    info[0] = c->sp.nS;
    info[1] = c->sp.nS ? c->sp.inert : -1;
    info[2] = speciesBatchWidth();
    info[3] = c->spKeep ? 1 : 0;
    return QGD_OK;
}

// one flux-assembly pass (updateFields.H + updateFluxes.H) on the current state; part 0 = all of it, 1 = up to p's mid-step boundary
// conditions, 2 = the rest.  A shard whose GaussVolPoint stencil meets a qgdFlux wall exchanges the mid-step patch pressure of the
// boundary layer's patch faces between 1 and 2 (midExchangeNeeded): a ghost cell's patch face forms it from an incomplete stencil, and the
// vertex values of p on the wall carry it into the stencil of owned faces.
static void assembleFluxes(qgd_case_s* c, bool adjust, int part = 0, bool internalFaces = true) {
    // internalFaces = false: the fused step computes them itself (stepFused)
    (void)hipGetLastError();  // drop any stale sticky error: the callers check after their launches
    const Launcher L = launcherOf(c);
    const MeshView& m = c->dev->view;
    const CaseView& v = c->view;
    const bool mid = c->pRefresh && c->hasQgdFlux;
    auto bface = [&](int phiwOnly, bool adj) {
        if (c->mixB >= 0) launchBoundaryFaceFluxMixed(L, c->stencil, c->mixB, c->mixMask, m, v, c->gas, c->bcDev, phiwOnly, adj);
        else launchBoundaryFaceFlux(L, c->stencil, m, v, c->gas, c->bcDev, phiwOnly, adj);
    };
    if (part != 2 && c->usesPoints) {
        if (internalFaces) launchPointInterp(L, m, v);   // (the fused kernel forms the vertex values of its blocks itself; patch points below)
        launchBoundaryPoints(L, m, v, false);
        // fvsc::grad(p) under GaussVolPoint re-runs p's BCs after phiwStar was refreshed
        // [QGDFoam/updateFluxes.H L63-65, GaussVolPointStencil_8C L73]
        if (mid) bface(1, false);  // + the mid-step pressure itself
    }
    if (part == 1) return;
    c->fluxAssembled = true;
    if (mid) launchBoundaryPoints(L, m, v, true);
    if (!internalFaces) {}
    else if (c->mixB >= 0) launchFaceFluxMixed(L, c->stencil, c->mixB, c->mixMask, m, v, c->gas, adjust);
    else launchFaceFlux(L, c->stencil, m, v, c->gas, adjust);
    bface(mid ? 2 : 0, adjust);
    // Courant-number control on the cell blocks: every block up to its cells' flux sums and its faces' Courant partials (the patch faces'
    // fluxes are in place now); the cells advance in stepAdvance, once deltaT is known
    if (c->fusedAdj && !internalFaces && !c->view.dbg) launchFusedAdjust(L, m, v, c->gas);
}
static bool midExchangeNeeded(const qgd_case_s* c) { return c->dev->sharded() && c->pRefresh && c->hasQgdFlux; }
// ---- the halo messages of the QGD case -------------------------------------------------------------------------------------
// kind 0: the state message, QGD_HALO_CELL_DOUBLES_HOST doubles per cell (RecA, RecB), 12 per boundary face (RecA, RecB, p gradient, lagged rho);
//         a case with species and QGD_SPECIES_HALO appends nS planes of one double per cell (qgd_species.hip caseSpeciesHaloKernel);
// kinds 1..4: the implicitDiffusion branch's own (1 grad U, 2 U, 3 search direction, 4 guess: implicitHaloWidth doubles per cell);
// kind 5: the message between step phases 5 and 6 (see assembleFluxes), 2 doubles per patch face of the slot's boundary-layer cells
static int caseHaloMove(qgd_case_s* c, int slot, int kind, double* buf, bool pack, hipStream_t stream) {
    qgd_device_s* d = c->dev;
    if (slot >= (int)d->halo.size()) return QGD_OK;  // an unsharded mesh has no slots: nothing to exchange
    const qgd_device_s::HaloSlot& h = d->halo[slot];
    const int32_t *cells = pack ? h.send : h.ghost, *faces = pack ? h.sendBF : h.ghostBF;
    const int32_t nCells = pack ? h.nSend : h.nGhost, nFaces = pack ? h.nSendBF : h.nGhostBF;
    if ((kind == 5 ? nFaces : nCells) == 0) return QGD_OK;
    if (!buf) return fail(QGD_ERR_INVALID, "null buffer");
    (void)hipGetLastError();   // a stale error of an earlier, refused call must not be taken for this launch's
    if (kind == 0) {
        Launcher L = launcherOf(c);
        L.pre = nullptr; L.post = nullptr; L.stream = stream;
        launchHaloPack(L, c->view, c->gas, cells, nCells, faces, nFaces, buf, pack);
        // the species tail behind the flow's part, which keeps its layout; on the same stream: the patch values follow the cells' Y
        if (c->spHalo)
            launchSpeciesHalo(stream, d->view, c->sp, cells, nCells, faces, nFaces,
                              buf + (size_t)QGD_HALO_CELL_DOUBLES_HOST * (size_t)nCells + 12 * (size_t)nFaces, pack);
    } else if (kind == 5) launchMidHalo(stream, c->view, faces, nFaces, buf, pack);
    else launchImplicitHalo(stream, d->view, c->view, c->impl, c->implSolver, kind, cells, nCells, buf, pack);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
}
// forCount: kinds 3 and 4 with room for the widest solve (what a caller sizes its buffers by); what is SENT has the width of the solve in flight
static HaloMessage haloMessage(qgd_case_s* c, int kind, bool forCount = false) {
    HaloMessage m;
    if (kind == 0) { m.perCell = QGD_HALO_CELL_DOUBLES_HOST + (c->spHalo ? c->sp.nS : 0); m.perFace = 12; }
    else if (kind == 5) m.perFace = 2;
    else m.perCell = (forCount && kind >= 3) ? 3 : implicitHaloWidth(c->implSolver, kind);
    m.move = [c, kind](int slot, double* buf, bool pack, hipStream_t stream) { return caseHaloMove(c, slot, kind, buf, pack, stream); };
    return m;
}
static HaloBuffers& haloBuffers(qgd_case_s* c) {
    c->haloBuf.arena = &c->arena;
    c->haloBuf.widest.perCell = c->implSolver ? 9 : QGD_HALO_CELL_DOUBLES_HOST;   // grad U: 9 per cell; state: 8 per cell and ...
    if (c->spHalo) c->haloBuf.widest.perCell = std::max(c->haloBuf.widest.perCell, QGD_HALO_CELL_DOUBLES_HOST + (int)c->sp.nS);   // (+ the species' planes)
    c->haloBuf.widest.perFace = 12;                                               // ... 12 per face
    return c->haloBuf;
}
// ---- native halo transport: RCCL send/recv inside the library -----------------------------------------------------------
// Replaces, for a C++/MPI host, what the reference does per gradient call with PstreamBuffers
// [extendedFaceStencilScalarGrad_8C L145-233] and with processor-patch evaluation [GaussVolPointStencil_8C L73]:
// ONE grouped send/recv pair per neighbouring rank per step, device buffers, stream-ordered, no host synchronisation.
extern "C++" {
namespace {
struct Rccl {
    void* lib = nullptr;
    decltype(&ncclGetUniqueId) getUniqueId = nullptr;
    decltype(&ncclCommInitRank) commInitRank = nullptr;
    decltype(&ncclCommDestroy) commDestroy = nullptr;
    decltype(&ncclSend) send = nullptr;
    decltype(&ncclRecv) recv = nullptr;
    decltype(&ncclAllReduce) allReduce = nullptr;
    decltype(&ncclGroupStart) groupStart = nullptr;
    decltype(&ncclGroupEnd) groupEnd = nullptr;
    decltype(&ncclGetErrorString) errorString = nullptr;
    decltype(&ncclCommCount) commCount = nullptr;
    decltype(&ncclCommUserRank) commUserRank = nullptr;
    decltype(&ncclCommCuDevice) commCuDevice = nullptr;
    std::string why;
};
Rccl& rcclRef() {
    static Rccl r;
    static bool tried = false;
    if (tried) return r;
    tried = true;
    // an RCCL already in the process (e.g. the one torch.distributed brought) is reused; otherwise the ROCm one is loaded
    const char* env = std::getenv("QGD_RCCL_LIB");
    const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names) {
        if (!n) continue;
        r.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        if (r.lib) break;
    }
    for (const char* n : names) {
        if (r.lib) break;
        if (!n) continue;
        r.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    }
    if (!r.lib) { r.why = "RCCL not found (librccl.so; set QGD_RCCL_LIB)"; return r; }
    auto sym = [&](const char* name) { void* p = dlsym(r.lib, name); if (!p && r.why.empty()) r.why = std::string("RCCL symbol missing: ") + name; return p; };
    r.getUniqueId = (decltype(r.getUniqueId))sym("ncclGetUniqueId");
    r.commInitRank = (decltype(r.commInitRank))sym("ncclCommInitRank");
    r.commDestroy = (decltype(r.commDestroy))sym("ncclCommDestroy");
    r.send = (decltype(r.send))sym("ncclSend");
    r.recv = (decltype(r.recv))sym("ncclRecv");
    r.allReduce = (decltype(r.allReduce))sym("ncclAllReduce");
    r.groupStart = (decltype(r.groupStart))sym("ncclGroupStart");
    r.groupEnd = (decltype(r.groupEnd))sym("ncclGroupEnd");
    r.errorString = (decltype(r.errorString))sym("ncclGetErrorString");
    r.commCount = (decltype(r.commCount))sym("ncclCommCount");
    r.commUserRank = (decltype(r.commUserRank))sym("ncclCommUserRank");
    r.commCuDevice = (decltype(r.commCuDevice))sym("ncclCommCuDevice");
    return r;
}
}  // namespace
}  // extern "C++"
struct qgd_comm_s {
    ncclComm_t comm = nullptr;
    int rank = 0, nRanks = 1, deviceId = 0;
};
#define RCCL_CHECK(expr)                                                                                          \
    do {                                                                                                          \
        ncclResult_t _r = (expr);                                                                                 \
        if (_r != ncclSuccess)                                                                                    \
            throw HipError(std::string(#expr) + ": " + (rcclRef().errorString ? rcclRef().errorString(_r) : "RCCL error")); \
    } while (0)
// RCCL matches the messages of one peer in issue order, and both sides issue in their own slot order: two slots towards
// the same rank (two ranks on a periodic cut, two disjoint interfaces with one neighbour) would land in each other's
// ghost lists.  Refused; a rank exchanging with itself (the one-GPU test of this path) is the one ordered exception.
// Called by every exchange AND at the top of the sharded step entries, before the first message of a step is issued
// (the mid-assembly message and the messages inside the implicit solves come before the state message).
static void checkHaloPeers(const qgd_comm_s* comm, const int32_t* peers, int n) {
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (peers[a] >= 0 && peers[a] == peers[b] && peers[a] != comm->rank)
                throw std::invalid_argument("halo exchange: rank " + std::to_string(peers[a]) + " is the peer of two halo slots; "
                                            "one slot per neighbouring rank (qgd_mesh_shard builds them that way)");
    for (int s = 0; s < n; ++s)
        if (peers[s] >= comm->nRanks) throw std::invalid_argument("halo exchange: peer rank out of range");
}
// THE halo exchange of both case types and every message kind, on `stream`: every slot with a neighbour packs its message into the case's
// send buffer, the messages travel, every such slot unpacks what arrived.  comm != nullptr: a grouped ncclSend / ncclRecv pair per slot
// towards peers[slot] (< 0: no neighbour).  comm == nullptr: the cyclic pairs of a periodic device, where slot s takes what its partner
// slot haloSelf[s] of the same case packed (peers is not read).
static void exchangeOn(qgd_device_s* d, qgd_comm_s* comm, const int32_t* peers, int nSlots, hipStream_t stream, const HaloMessage& msg,
                       HaloBuffers& bufs) {
    const int n = std::min<int>(nSlots, (int)d->halo.size());
    if (comm) checkHaloPeers(comm, peers, n);
    bufs.ensure(d);
    auto move = [&](int s, double* buf, bool pack) {
        if ((!comm || peers[s] >= 0) && msg.move(s, buf, pack, stream) != QGD_OK) throw std::invalid_argument(g_lastError);
    };
    for (int s = 0; s < n; ++s) move(s, bufs.send[s], true);
    if (comm) {
        RCCL_CHECK(rcclRef().groupStart());
        try {
            for (int s = 0; s < n; ++s) {
                if (peers[s] < 0) continue;
                const size_t ns = msg.sendCount(d->halo[s]), nr = msg.recvCount(d->halo[s]);
                if (ns) RCCL_CHECK(rcclRef().send(bufs.send[s], ns, ncclFloat64, peers[s], comm->comm, stream));
                if (nr) RCCL_CHECK(rcclRef().recv(bufs.recv[s], nr, ncclFloat64, peers[s], comm->comm, stream));
            }
        } catch (...) {
            (void)rcclRef().groupEnd();   // never leave the group open behind a failed call: the next collective would join it
            throw;
        }
        RCCL_CHECK(rcclRef().groupEnd());
    } else {
        for (int s = 0; s < n; ++s)
            if (d->halo[(size_t)d->haloSelf[s]].nSend != d->halo[s].nGhost || d->halo[(size_t)d->haloSelf[s]].nSendBF != d->halo[s].nGhostBF)
                throw std::runtime_error("cyclic self-exchange: a slot's ghosts do not match its partner's message");
    }
    for (int s = 0; s < n; ++s) move(s, comm ? bufs.recv[s] : bufs.send[(size_t)d->haloSelf[s]], false);
}
static void exchangeOn(qgd_case_s* c, qgd_comm_s* comm, const int32_t* peers, int nSlots, hipStream_t stream, int kind) {
    exchangeOn(c->dev, comm, peers, nSlots, stream, haloMessage(c, kind), haloBuffers(c));
}
// cyclic pairs served by ghost cells: what a rank does with its neighbours, with itself (mid = the message in the middle of the assembly)
static void selfHaloExchange(qgd_case_s* c, bool mid) { exchangeOn(c, nullptr, nullptr, (int)c->dev->halo.size(), c->stream(), mid ? 5 : 0); }

int qgd_case_set_fields(qgd_case_t c, const double* U, const double* T, const double* p) {
    QGD_TRY
    if (!c || !U || !T || !p) return fail(QGD_ERR_INVALID, "qgd_case_set_fields: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MeshView& m = c->dev->view;
    c->hasQgdFlux = false;
    for (const PatchBCDev& b : c->bc) if (b.bcP == QGD_BC_QGDFLUX) c->hasQgdFlux = true;
    if (!c->bc.empty()) HIP_CHECK(hipMemcpy(c->bcDev, c->bc.data(), sizeof(PatchBCDev) * c->bc.size(), hipMemcpyHostToDevice));
    double *dU = nullptr, *dT = nullptr, *dp = nullptr;
    auto cleanup = [&]() { (void)hipFree(dU); (void)hipFree(dT); (void)hipFree(dp); };
    try {
        HIP_CHECK(hipMalloc((void**)&dU, sizeof(double) * 3 * (size_t)m.nC));
        HIP_CHECK(hipMalloc((void**)&dT, sizeof(double) * (size_t)m.nC));
        HIP_CHECK(hipMalloc((void**)&dp, sizeof(double) * (size_t)m.nC));
        HIP_CHECK(hipMemcpy(dU, U, sizeof(double) * 3 * (size_t)m.nC, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dT, T, sizeof(double) * (size_t)m.nC, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dp, p, sizeof(double) * (size_t)m.nC, hipMemcpyHostToDevice));
        Launcher L = launcherOf(c);
        L.pre = nullptr; L.post = nullptr;
        (void)hipGetLastError();
        launchCellInit(L, m, c->view, c->gas, dU, dT, dp);
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, true, false, 0, nullptr, 0);
        if (c->varSc) launchVarSc7(L, m, c->view, c->gas, c->vsc, true);   // the thermo object's constructor runs the model once, on the evaluated patch pressures
        launchResetReductions(L, c->view);
        if (c->fused) {   // a shard's ghost records are written by the halo exchange only: both buffers start with the initial ones
            HIP_CHECK(hipMemcpyAsync(c->view.A2, c->view.A, sizeof(RecA) * (size_t)m.nC, hipMemcpyDeviceToDevice, c->stream()));
            HIP_CHECK(hipMemcpyAsync(c->view.B2, c->view.B, sizeof(RecB) * (size_t)m.nC, hipMemcpyDeviceToDevice, c->stream()));
        }
        const double dt0[3] = {c->opt.deltaT, 0.0, 0.0};
        HIP_CHECK(hipMemcpyAsync(c->view.dt, dt0, sizeof(dt0), hipMemcpyHostToDevice, c->stream()));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream()));
    } catch (...) { cleanup(); throw; }
    cleanup();
    c->phiwRegistered = true;  // createFaceFluxes.H registers "phiwStar" before the loop starts
    c->ghostsCurrent = false;  // (cyclic pairs served by ghost cells: the copies take their originals' records before the first step)
    c->fieldsSet = true;
    c->fluxAssembled = false;
    c->spFluxesValid = false;  // (the species fluxes kept from a step before this call are no longer "the last step's")
    c->gradUValid = false;
    c->impl.have = 0;          // the start values of the implicit solves begin without a history
    c->time = 0; c->steps = 0;
    if (c->spStats) HIP_CHECK(hipMemsetAsync(c->spStats, 0, sizeof(double) * (size_t)implicitStatsDoubles(c->spBatches), c->stream()));
    if (c->implSolver) { implicitSolverSetStream(c->implSolver, c->stream()); implicitStatsReset(c->implSolver); HIP_CHECK(hipStreamSynchronize(c->stream())); }
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_update_fluxes(qgd_case_t c) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_update_fluxes: call qgd_case_set_fields first");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MeshView& m = c->dev->view;
    if (!c->dbgBuf) c->dbgBuf = c->arena.alloc<double>((size_t)DBG_COUNT * m.nF);
    HIP_CHECK(hipMemsetAsync(c->dbgBuf, 0, sizeof(double) * (size_t)DBG_COUNT * m.nF, c->stream()));
    c->view.dbg = c->dbgBuf;
    if (c->dev->periodic()) {
        // cyclic pairs served by ghost cells: the copies belong to the library, whatever the caller put into them with set_fields -- they take
        // their originals' records before anything is computed from them (and the mid-step message where qgd_case_step has one)
        if (c->sp.nS && !c->ghostsCurrent) { const int rs = speciesReady(c, "qgd_case_update_fluxes"); if (rs) return rs; }   // (the refresh moves the composition too)
        if (!c->ghostsCurrent) { selfHaloExchange(c, false); c->ghostsCurrent = true; }
        if (midExchangeNeeded(c)) { assembleFluxes(c, false, 1); selfHaloExchange(c, true); assembleFluxes(c, false, 2); }
        else assembleFluxes(c, false);
    } else assembleFluxes(c, false);
    c->view.dbg = nullptr;
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    return QGD_OK;
    QGD_CATCH
}

// phase 0: flux assembly (+ the shard's max Cof / min tauQGDf into red[0], -red[1]);
// phase 1: deltaT, cell update, boundary refresh
static void stepAssemble(qgd_case_s* c, int part = 0) {
    const bool adjust = c->opt.adjustTimeStep != 0;
    assembleFluxes(c, adjust, part, !(c->fused || implFusedNow(c) || c->fusedAdj));   // a fused case computes its internal faces inside the advance (stepAdvance / phase 21)
    if (adjust && part != 1) launchFaceReduce(launcherOf(c), c->view);
}
// ---- the implicitDiffusion branch [QGDUEqn.H L54-75, QGDEEqn.H L53-64] as stream-ordered phases ---------------------------------
//   20  deltaT, fvc::grad(U) of the old state                                -> message kind 1
//   21  tauMC / phiTauMC, rho, rhoU, the three U systems and their start values -> message kind 4
//   22  solver phase 0 (A x, r)                                              -> reduce control slots 0..2
//   23, 24  solver phases 1, 2                                               -> reduce slot 3 | slot 4 + message kind 3
//   25, 26, 27  one PCG iteration (solver phases 3, 4, 5)                     -> reduce slot 5 | slots 6..7 | message kind 3
//   28  U into the records, its boundary conditions                          -> message kind 2
//   29  fvc::grad(U) of the new velocity                                     -> message kind 1
//   30  phiSigmaDotU, the energy equation's explicit part, the e system       -> message kind 4; then 22, 23, 24, (25, 26, 27)* for e
//   35  rhoE, thermo, p, boundary refresh                                    -> the state message (qgd_case_halo_*)
// No host synchronisation anywhere inside.
static void implicitPhase(qgd_case_s* c, int phase) {
    const qgd_device_s* d = c->dev;
    const MeshView& m = d->view;
    ImplicitSolver* S = c->implSolver;
    hipStream_t st = c->stream();
    implicitSolverSetStream(S, st);
    const double tol = c->opt.implicitTol;
    const int maxIter = c->opt.implicitMaxIter;
    (void)hipGetLastError();
    switch (phase) {
        case 20: {
            const bool adjust = c->opt.adjustTimeStep != 0;
            if (c->varSc) launchVarSc7(launcherOf(c), m, c->view, c->gas, c->vsc, false);   // thermo.correct() of this step sees the pressures the step starts with
            if (adjust) launchDeltaT(launcherOf(c), c->view, c->opt.maxCo, c->opt.maxDeltaT, c->opt.cTau);
            if (adjust) launchImplicitStartWeights(st, c->view, c->impl);   // the start values' Lagrange weights from the deltaT ratios
            c->steps++;
            if (!adjust) c->time += c->opt.deltaT;
            implicitStepMark(S, true);
            // fvc::grad(U) of the state before the step IS the gradient phase 29 of the step before formed from the new velocity and its
            // patch values: nothing has touched either since (unsharded; any field, BC or coefficient upload resets the flag)
            if (!(c->reuseGradU && c->gradUValid && !d->sharded())) launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 0);
            c->gradUValid = false;
            break;
        }
        case 21: c->implSolveIndex = 0; launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 1, implFusedNow(c)); break;
        case 22: case 23: case 24: case 25: case 26: case 27: implicitSolvePhase(S, phase - 22); break;
        case 28:
            implicitSolveEnd(S, 0);
            launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 2);
            break;
        case 29: launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 3); c->gradUValid = true; break;
        case 30: c->implSolveIndex = 1; launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 4); break;
        case 35:
            implicitSolveEnd(S, 1);
            launchImplicitPart(st, m, c->view, c->impl, c->gas, c->bcDev, S, tol, maxIter, 5);
            if (c->impl.pred) {   // this step's corrections sit in the oldest slot: it becomes the newest
                ImplView& iv = c->impl;
                double* t = iv.dh[iv.order - 1];
                for (int j = iv.order - 1; j >= 1; --j) iv.dh[j] = iv.dh[j - 1];
                iv.dh[0] = t;
                iv.have = std::min(iv.have + 1, iv.order);
            }
            implicitStepMark(S, false);
            launchBoundaryUpdate(launcherOf(c), m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, 0, nullptr, 0);
            break;
        default: throw std::invalid_argument("implicit branch: phase must be 20..30 or 35");
    }
    HIP_CHECK(hipGetLastError());
}
// the whole advance with the transport behind the hooks (nullptr: one rank); haloImpl(kind) exchanges message kind 1 / 2
static void implicitAdvanceWith(qgd_case_s* c, const SolveHooks* hooks, const std::function<void(int)>& haloImpl) {
    ImplicitSolver* S = c->implSolver;
    implicitPhase(c, 20);
    if (haloImpl) haloImpl(1);
    if (c->sp.nS) {
        // the species block [reactingLagrangianQGDFoam_8C L92-140: the species fluxes, QGDRhoEqn, QGDYEqn L47-66, then QGDUEqn, QGDEEqn]: the
        // records still hold the state before the step (phase 28 writes rho and U), deltaT is this step's (phase 20), plane 0 of the flux
        // is the assembled mass flux of every face (a case with species takes the separate assembly kernels)
        (void)hipGetLastError();
        launchSpeciesAdvanceImplicit(c->stream(), c->stencil, c->dev->view, c->view, c->gas, c->sp, c->spImpl, S,
                                     c->spTol > 0 ? c->spTol : c->opt.implicitTol, c->spMaxIter > 0 ? c->spMaxIter : c->opt.implicitMaxIter, c->spStats);
        HIP_CHECK(hipGetLastError());
        c->spFluxesValid = true;
    }
    implicitPhase(c, 21);
    implicitSolveRun(S, hooks);     // message kind 4, phase 0, ... through the hooks
    implicitPhase(c, 28);
    if (haloImpl) haloImpl(2);
    implicitPhase(c, 29);
    if (haloImpl) haloImpl(1);
    implicitPhase(c, 30);
    implicitSolveRun(S, hooks);
    implicitPhase(c, 35);
}

// part 0 = everything; part 1 = deltaT + the shard's boundary layer (cells a neighbour needs, and their patch faces);
// part 2 = the remaining owned cells/faces.  Ghost cells and their patch faces are only ever written by halo_unpack.
static void stepAdvance(qgd_case_s* c, int part) {
    const Launcher L = launcherOf(c);
    const qgd_device_s* d = c->dev;
    const MeshView& m = d->view;
    const bool adjust = c->opt.adjustTimeStep != 0;
    if (c->opt.implicitDiffusion) {
        implicitAdvanceWith(c, nullptr, nullptr);   // deltaT and the step count are advanced inside (phase 20)
        return;
    }
    if (part != 2) {
        // varScModel7: the Schmidt numbers thermo.correct() of this step forms, from the pressures the step starts with (every owned cell, ahead
        // of the boundary layer's advance: the cell update writes p in place)
        if (c->varSc) launchVarSc7(L, m, c->view, c->gas, c->vsc, false);
        if (adjust) launchDeltaT(L, c->view, c->opt.maxCo, c->opt.maxDeltaT, c->opt.cTau);
        c->steps++;
        if (!adjust) c->time += c->opt.deltaT;
    }
    if (c->fusedAdj) {
        launchCellFinish(L, m, c->view, c->gas, part, part == 1 ? d->sendAll : nullptr, part == 1 ? d->nSendAll : 0);
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, part,
                             part == 1 ? d->sendBFAll : nullptr, part == 1 ? d->nSendBFAll : 0);
        return;
    }
    if (c->fused) {
        // The fused face + cell kernel writes the new records to A2 / B2 (its blocks read their neighbours' OLD records), which then become
        // A / B.  On a shard the boundary-layer blocks go first (part 1) and the swap follows them at once, so that the halo pack and the
        // patch faces of those cells see the new records; the remaining blocks (part 2) then read the old records where the swap left
        // them -- A2 / B2 -- and write where the new ones belong.
        if (part == 0) {
            launchFusedFaceCell(L, m, c->view, c->gas, 0, m.fuBlocks);
            std::swap(c->view.A, c->view.A2);
            std::swap(c->view.B, c->view.B2);
        } else if (part == 1) {
            launchFusedFaceCell(L, m, c->view, c->gas, 0, m.fuLayerBlocks);
            std::swap(c->view.A, c->view.A2);
            std::swap(c->view.B, c->view.B2);
        } else {
            CaseView back = c->view;
            std::swap(back.A, back.A2);
            std::swap(back.B, back.B2);
            launchFusedFaceCell(L, m, back, c->gas, m.fuLayerBlocks, m.fuBlocks - m.fuLayerBlocks);
        }
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, part,
                             part == 1 ? d->sendBFAll : nullptr, part == 1 ? d->nSendBFAll : 0);
        return;
    }
    if (part == 0) {
        // the species block reads the old records, the assembled mass flux and this step's deltaT: ahead of the flow's cell update
        // [reactingLagrangianQGDFoam_8C L92-140: QGDRhoEqn, QGDYEqn, QGDUEqn, QGDEEqn]
        if (c->sp.nS) { launchSpeciesAdvance(L.stream, c->stencil, m, c->view, c->gas, c->sp); c->spFluxesValid = true; }
        launchCellUpdate(L, m, c->view, c->gas, 0, nullptr, 0);
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, 0, nullptr, 0);
    } else if (part == 1) {
        // The species on a shard, boundary layer first.  Part 1 runs the vertex values and BOTH face kernels over ALL faces -- they read the
        // old records and the old Y of both sides, which nothing has touched yet -- then the species' cell and patch kernels on the layer,
        // ahead of the flow's, which overwrites the layer's records.  Part 2 can then run beside the unpack of the state message on the
        // halo stream: it reads SpeciesView::F and CaseView::flux (complete since part 1 / the assembly, written by neither), and the
        // records, Y and patch faces of ordinary owned cells only, and writes Y and Y.boundary of those alone; the unpack writes the
        // records, Y and patch values of GHOST cells alone, the pack reads those of the layer alone.  No kernel of part 2 reads or writes
        // what the concurrent exchange writes or reads.
        if (c->sp.nS) {
            launchSpeciesAdvance(L.stream, c->stencil, m, c->view, c->gas, c->sp, 1, d->sendAll, d->nSendAll, d->sendBFAll, d->nSendBFAll);
            c->spFluxesValid = true;
        }
        launchCellUpdate(L, m, c->view, c->gas, 1, d->sendAll, d->nSendAll);
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, 1, d->sendBFAll, d->nSendBFAll);
    } else {
        if (c->sp.nS) launchSpeciesAdvance(L.stream, c->stencil, m, c->view, c->gas, c->sp, 2);
        launchCellUpdate(L, m, c->view, c->gas, 2, nullptr, 0);
        launchBoundaryUpdate(L, m, c->view, c->gas, c->bcDev, false, c->phiwRegistered, 2, nullptr, 0);
    }
}

int qgd_case_step(qgd_case_t c, int32_t nSteps) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_step: call qgd_case_set_fields first");
    if (c->dev->sharded() && !c->dev->periodic())
        return fail(QGD_ERR_INVALID, "qgd_case_step: sharded mesh, drive it with qgd_case_step_phase + halo exchange");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    if (c->dev->periodic()) {
        // cyclic pairs served by ghost cells: the copies are refreshed from their originals after every step (and in the middle of the
        // assembly where a shard would exchange there), all on the case's stream -- what a rank does with its neighbours, with itself
        if (c->opt.implicitDiffusion)
            return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_step: the implicitDiffusion branch on a mesh with cyclic patches (qgd_mesh_unroll_cyclic) is not served: "
                                                 "its solves would need the coupled rows; use the explicit branch");
        // (the species' boundary-condition tables reach the device first: the refresh re-evaluates the copies' patch values from them)
        if (c->sp.nS) { const int rs = speciesReady(c, "qgd_case_step"); if (rs) return rs; }
        if (!c->ghostsCurrent) { selfHaloExchange(c, false); c->ghostsCurrent = true; }
        for (int i = 0; i < nSteps; ++i) {
            if (midExchangeNeeded(c)) { stepAssemble(c, 1); selfHaloExchange(c, true); stepAssemble(c, 2); }
            else stepAssemble(c);
            if (c->opt.adjustTimeStep) {}   // (one rank: the shard's own maximum IS the global one)
            stepAdvance(c, 0);
            selfHaloExchange(c, false);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream()));
        return QGD_OK;
    }
    if (c->sp.nS) { const int rs = speciesReady(c, "qgd_case_step"); if (rs) return rs; }
    for (int i = 0; i < nSteps; ++i) { stepAssemble(c); stepAdvance(c, 0); }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_step_phase(qgd_case_t c, int phase) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_step_phase: call qgd_case_set_fields first");
    // (a case with species and QGD_SPECIES_HALO on a cell-range shard advances through the phases like any other; a periodic device is sharded() too)
    const bool speciesPhases = c->sp.nS && c->spHalo && c->dev->sharded() && !c->dev->periodic() && !c->opt.implicitDiffusion &&
                               (phase == 0 || phase == 1 || phase == 2 || phase == 5 || phase == 6 || phase == 10 || phase == 11);
    if (c->sp.nS && !speciesPhases)
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_step_phase: the case carries species (qgd_case_set_species), which advance inside qgd_case_step only");
    if (c->dev->periodic())
        return fail(QGD_ERR_INVALID, "qgd_case_step_phase: a periodic device (cyclic patches served by ghost copies, qgd_mesh_unroll_cyclic) is stepped with "
                                     "qgd_case_step, which refreshes the copies after every step; a phase would compute on stale copies");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    if (c->opt.implicitDiffusion && (phase == 10 || phase == 11))
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_case_step_phase: the implicitDiffusion branch has no boundary-layer-first order (its linear "
                                            "solves span all cells); use phases 0 and 1, or 0 and 20..30, 35 on a shard");
    if (phase >= 20 && phase <= 35) {
        if (!c->opt.implicitDiffusion) return fail(QGD_ERR_INVALID, "qgd_case_step_phase: phases 20..35 belong to the implicitDiffusion branch");
        if ((phase > 30 && phase < 35)) return fail(QGD_ERR_INVALID, "qgd_case_step_phase: phase must be 0, 1, 2, 10, 11, 20..30 or 35");
        implicitPhase(c, phase);
        return QGD_OK;
    }
    if (c->opt.implicitDiffusion && phase == 1 && c->dev->sharded())
        return fail(QGD_ERR_INVALID, "qgd_case_step_phase: on a shard the implicitDiffusion branch advances through phases 20..35 with the "
                                     "exchanges between them");
    if (c->sp.nS && (phase == 0 || phase == 5)) { const int rs = speciesReady(c, "qgd_case_step_phase"); if (rs) return rs; }   // where a step begins
    if (phase == 0) stepAssemble(c);
    else if (phase == 5) stepAssemble(c, 1);
    else if (phase == 6) stepAssemble(c, 2);
    else if (phase == 1) stepAdvance(c, 0);
    else if (phase == 10) stepAdvance(c, 1);
    else if (phase == 11) stepAdvance(c, 2);
    else if (phase == 3) {
        if (c->dev->sharded()) return fail(QGD_ERR_INVALID, "qgd_case_step_phase: phase 3 (one whole step, no exchange) is for unsharded meshes");
        stepAssemble(c);
        stepAdvance(c, 0);
    } else if (phase != 2) return fail(QGD_ERR_INVALID, "qgd_case_step_phase: phase must be 0, 1, 2, 3, 5, 6, 10 or 11");
    HIP_CHECK(hipGetLastError());
    return QGD_OK;  // asynchronous: qgd_case_stream_sync waits
    QGD_CATCH
}
int qgd_case_set_halo_stream(qgd_case_t c, void* hipStream) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    c->haloStream = (hipStream_t)hipStream;
    c->useHaloStream = true;
    return QGD_OK;
}
int qgd_case_reduction_ptr(qgd_case_t c, void** devicePtr) {
    if (!c || !devicePtr) return fail(QGD_ERR_INVALID, "null argument");
    *devicePtr = c->view.red;
    return QGD_OK;
}
int qgd_case_set_stream(qgd_case_t c, void* hipStream) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    (void)hipSetDevice(c->dev->deviceId);
    harvestTiming(c);
    (void)hipStreamSynchronize(c->stream());
    c->userStream = (hipStream_t)hipStream;
    c->useUserStream = true;
    return QGD_OK;
}
// the wait behind qgd_case_stream_sync, qgd_qhd_case_sync and qgd_scalar_case_sync
static int caseSync(CaseCore* c) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    return QGD_OK;
    QGD_CATCH
}
int qgd_case_stream_sync(qgd_case_t c) { return caseSync(c); }

int qgd_device_alloc(qgd_device_t d, int64_t bytes, void** devicePtr) {
    QGD_TRY
    if (!d || !devicePtr || bytes <= 0) return fail(QGD_ERR_INVALID, "qgd_device_alloc: bad argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipMalloc(devicePtr, (size_t)bytes));
    HIP_CHECK(hipMemset(*devicePtr, 0, (size_t)bytes));
    HIP_CHECK(hipStreamSynchronize(nullptr));   // the zero-fill is done before the caller's first copy on the device's (non-blocking) stream
    return QGD_OK;
    QGD_CATCH
}
int qgd_device_release(qgd_device_t d, void* devicePtr) {
    QGD_TRY
    if (!d) return fail(QGD_ERR_INVALID, "null device");
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipFree(devicePtr));
    return QGD_OK;
    QGD_CATCH
}

// ---- the public halo entries of both case kinds, after their own argument checks: the doubles of message m for a slot (none beyond the
// device's slots), and its pack / unpack on a stream
static int caseHaloCount(const CaseCore* c, int slot, const HaloMessage& m, int64_t* sendCount, int64_t* recvCount) {
    *sendCount = *recvCount = 0;
    if (slot >= (int)c->dev->halo.size()) return QGD_OK;
    *sendCount = (int64_t)m.sendCount(c->dev->halo[slot]);
    *recvCount = (int64_t)m.recvCount(c->dev->halo[slot]);
    return QGD_OK;
}
static int caseHaloMovePublic(const CaseCore* c, int slot, const HaloMessage& m, const double* buf, bool pack, hipStream_t stream) {
    QGD_TRY
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    return m.move(slot, const_cast<double*>(buf), pack, stream);
    QGD_CATCH
}
// of a QGD case: counts with room for the widest solve (haloMessage's forCount); the state message honours qgd_case_set_halo_stream, the
// others run on the case's stream
static int qgdHaloCount(qgd_case_s* c, int slot, int kind, int64_t* sendCount, int64_t* recvCount) {
    return caseHaloCount(c, slot, haloMessage(c, kind, true), sendCount, recvCount);
}
static int qgdHaloMove(qgd_case_s* c, int slot, int kind, const double* buf, bool pack) {
    return caseHaloMovePublic(c, slot, haloMessage(c, kind), buf, pack, kind == 0 && c->useHaloStream ? c->haloStream : c->stream());
}
int qgd_case_halo_count(qgd_case_t c, int slot, int64_t* count) {
    int64_t recv;
    if (!c || !count || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloCount(c, slot, 0, count, &recv);
}
int qgd_case_halo_recv_count(qgd_case_t c, int slot, int64_t* count) {
    int64_t send;
    if (!c || !count || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloCount(c, slot, 0, &send, count);
}
int qgd_case_halo_pack(qgd_case_t c, int slot, double* sendBufDevice) {
    if (!c || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, 0, sendBufDevice, true);
}
int qgd_case_halo_unpack(qgd_case_t c, int slot, const double* recvBufDevice) {
    if (!c || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, 0, recvBufDevice, false);
}
int qgd_case_mid_exchange_needed(qgd_case_t c, int32_t* needed) {
    if (!c || !needed) return fail(QGD_ERR_INVALID, "bad argument");
    *needed = midExchangeNeeded(c) ? 1 : 0;
    return QGD_OK;
}
int qgd_case_mid_halo_count(qgd_case_t c, int slot, int64_t* sendCount, int64_t* recvCount) {
    if (!c || slot < 0 || !sendCount || !recvCount) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloCount(c, slot, 5, sendCount, recvCount);
}
int qgd_case_mid_halo_pack(qgd_case_t c, int slot, double* sendBufDevice) {
    if (!c || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, 5, sendBufDevice, true);
}
int qgd_case_mid_halo_unpack(qgd_case_t c, int slot, const double* recvBufDevice) {
    if (!c || slot < 0) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, 5, recvBufDevice, false);
}
// the branch's own messages on a shard (kinds 1 grad U, 2 U, 3 search direction, 4 guess): counts in doubles
int qgd_case_implicit_halo_count(qgd_case_t c, int slot, int kind, int64_t* sendCount, int64_t* recvCount) {
    if (!c || slot < 0 || kind < 1 || kind > 4 || !sendCount || !recvCount) return fail(QGD_ERR_INVALID, "bad argument");
    *sendCount = *recvCount = 0;
    if (!c->implSolver) return fail(QGD_ERR_INVALID, "qgd_case_implicit_halo_count: not an implicitDiffusion case");
    return qgdHaloCount(c, slot, kind, sendCount, recvCount);
}
int qgd_case_implicit_halo_pack(qgd_case_t c, int slot, int kind, double* sendBufDevice) {
    if (!c || slot < 0 || kind < 1 || kind > 4 || !c->implSolver) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, kind, sendBufDevice, true);
}
int qgd_case_implicit_halo_unpack(qgd_case_t c, int slot, int kind, const double* recvBufDevice) {
    if (!c || slot < 0 || kind < 1 || kind > 4 || !c->implSolver) return fail(QGD_ERR_INVALID, "bad argument");
    return qgdHaloMove(c, slot, kind, recvBufDevice, false);
}

// ---- QHDFoam case resident on the device -------------------------------------------------------------------------------
struct qgd_qhd_case_s : CaseCore {   // (implSolver: the four systems {Ux, Uy, Uz, T} as one multi-right-hand-side solve; haloBuf: qgd_qhd_case_halo_exchange, qgd_qhd_case_step_sharded)
    qgd_qhd_options opt{};
    double* pHist[4] = {nullptr, nullptr, nullptr, nullptr}; int pOrder = 0, pPrevHave = 0;   // QGD_QHD_PEXTRAP: p of the steps before (start value of the pressure solve, qgd_qhd.hip)
    int implXOrder = 0;         // QGD_IMPL_XEXTRAP (QhdView::xHave counts up to it)   // QGD_QHD_PEXTRAP: p of the step before (start value of the pressure solve, qgd_qhd.hip)
    QhdView view{};
    double* c4b = nullptr;      // QGD_QHD_FUSED: the second {U,T} array of the block-fused U / T equations (qgd_qhd.hip qhdFusedAdvanceKernel); swapped with view.c4 every step
    double *tauF = nullptr, *tbr = nullptr, *scratch = nullptr;
    uint8_t* bKind = nullptr;
    PressureSolver* solver = nullptr;
    int implMask = 15;                     // components that are solved (validComponents: not those along empty directions)
    bool needRef = false;
    int localRefCell = -1;                 // local label of pRefCell when this shard owns it
    std::vector<int32_t> bcPRequested;     // p kinds as the caller set them (a box slab's cut plane hides the patch's own kind)
    double lastIter = 0, lastRes0 = 0, lastRes = 0, lastSolveMs = 0;
    double* bValUDev = nullptr;            // qgd_qhd_case_set_bc_values: 3 per boundary face (view.bValU while some patch's valList names U)
    // adjustTimeStep (qgd_qhd_case_set_time_control) [QHDCourantNo.H L37-57, setDeltaT-QGDQHD.H L41-61]: view.dt is the deltaT in force.
    // rShf: 1/(|Sf| hQGDf) per face; red: {max |phiu| rShf, min tauQGDf} on the device, redHost its pinned copy, read at the step's one wait
    bool adjust = false;
    double maxCo = 1.0, maxDeltaT = 1e300, cTau = 0.75;
    double *rShf = nullptr, *red = nullptr, *redHost = nullptr;
    double minTau = 0, maxUh = 0, CoNum = 0;   // of the last step whose maximum was reduced (coSteps == steps: valid for the last step)
    int64_t coSteps = -1;
    double dtDiag = 0;                     // implicitDiffusion: the deltaT view.diag4 was built with
    bool tcReady = false;                  // rShf and minTau stand for the fields of the last qgd_qhd_case_set_fields
    std::vector<double> dtHist;            // deltaT of the completed steps, newest first (start values under unequal steps)
    bool lagrange = true;                  // QGD_QHD_LAGRANGE (default 1; 0: the equal-step weights whatever the steps)
};
// Lagrange weights of the start value one step of length g0 ahead of the current field, through it and the k fields before it, which lie
// dtHist[first], dtHist[first + 1], ... apart (a gap from before the first step counts as the oldest known one).  false: the steps are
// equal -- the binomial weights of the kernels as they were, exactly -- or the case runs with QGD_QHD_LAGRANGE=0
static bool qhdStartWeights(const qgd_qhd_case_s* c, double g0, size_t first, int k, QhdStartWeights& W) {
    if (!c->lagrange || k < 1 || c->dtHist.empty()) return false;
    double s[5] = {0, 0, 0, 0, 0};
    bool equal = true;
    for (int j = 1; j <= k; ++j) {
        const double g = c->dtHist[std::min(first + (size_t)j - 1, c->dtHist.size() - 1)];
        equal = equal && g == g0;
        s[j] = s[j - 1] - g;
    }
    if (equal) return false;
    W.k = k;
    for (int i = 0; i < 5; ++i) {
        double w = i <= k ? 1.0 : 0.0;
        for (int j = 0; j <= k && i <= k; ++j) if (j != i) w *= (g0 - s[j]) / (s[i] - s[j]);
        W.w[i] = w;
    }
    return true;
}
// rShf and min(tauQGDf) [setDeltaT-QGDQHD.H L52-55], formed when the time controls are first asked for after qgd_qhd_case_set_fields: a
// case that never asks holds neither the 8 B per face nor launches anything for them
static void qhdTimeControlReady(qgd_qhd_case_s* c) {
    if (c->tcReady || !c->fieldsSet) return;
    qgd_device_s* d = c->dev;
    const MeshView& m = d->view;
    HIP_CHECK(hipSetDevice(d->deviceId));
    if (!c->rShf) { c->rShf = c->arena.alloc<double>(std::max<size_t>((size_t)m.nF, 1)); c->red = c->arena.alloc<double>(2); }
    if (!c->redHost) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&c->redHost), 2 * sizeof(double), hipHostMallocDefault));
    double red0[2] = {0.0, std::numeric_limits<double>::infinity()};
    (void)hipGetLastError();
    HIP_CHECK(hipMemcpyAsync(c->red, red0, sizeof(red0), hipMemcpyHostToDevice, d->stream));
    launchQhdTimeControlSetup(d->stream, m, c->tauF, c->rShf, c->red);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(red0, c->red, sizeof(red0), hipMemcpyDeviceToHost, d->stream));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    c->minTau = red0[1];
    c->tcReady = true;
}
// the step's maximum into redHost[0], stream-ordered: the caller waits for the stream before reading
static void qhdCourantQueue(qgd_qhd_case_s* c) {
    hipStream_t s = c->dev->stream;
    HIP_CHECK(hipMemsetAsync(c->red, 0, sizeof(double), s));
    launchQhdCourant(s, c->dev->view, c->view, c->rShf, c->red);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(c->redHost, c->red, sizeof(double), hipMemcpyDeviceToHost, s));
}
// setDeltaT-QGDQHD.H L41-61 on the maximum just read: the deltaT of the U and T equations of this step
static void qhdSetDeltaT(qgd_qhd_case_s* c) {
    double& dt = c->view.dt;
    c->maxUh = std::max(c->redHost[0], 0.0);
    c->CoNum = dt * c->maxUh;                                                     // QHDCourantNo.H L44-48
    c->coSteps = c->steps + 1;
    const double maxDeltaTFact = c->maxCo / (c->CoNum + 1e-15);
    const double deltaTFact = std::min(std::min(maxDeltaTFact, 1.0 + 0.1 * maxDeltaTFact), 1.2);
    dt = std::min(deltaTFact * dt, std::min(c->maxDeltaT, c->cTau * c->minTau));
}

int qgd_qhd_options_default(qgd_qhd_options* o) {
    if (!o) return fail(QGD_ERR_INVALID, "null argument");
    std::memset(o, 0, sizeof(*o));
    o->stencil = QGD_FVSC_GAUSSVOLPOINT;
    o->tauModel = 2; o->pRefCell = 0; o->pMaxIter = 1000; o->precond = 1;
    o->rho0 = 1.0; o->mu = 1e-3; o->Pr = 0.71; o->beta = 3e-3; o->g[1] = -9.81; o->deltaT = 1e-3;
    o->Tau = 1e-3; o->aQGD = 0.5; o->UQHD = 1.0; o->T0 = 1.0; o->Gr = 1e3; o->pTol = 1e-8; o->pRelTol = 0.0; o->pRefValue = 0.0;
    o->implicitTol = 1e-10; o->implicitMaxIter = 1000;
    return QGD_OK;
}
int qgd_qhd_case_create(qgd_device_t d, const qgd_qhd_options* opt, qgd_qhd_case_t* out) {
    QGD_TRY
    if (!d || !opt || !out) return fail(QGD_ERR_INVALID, "qgd_qhd_case_create: null argument");
    if (d->periodic())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_case_create: a mesh whose cyclic patches were unrolled into ghost cells (qgd_mesh_unroll_cyclic) is served by "
                                             "QGDFoam's explicit branch only: the pressure equation would need the coupled rows");
    if (opt->implicitDiffusion && (!(opt->implicitTol > 0) || opt->implicitMaxIter < 1))
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_create: implicitDiffusion needs implicitTol > 0 and implicitMaxIter >= 1");
    if (!(opt->rho0 > 0) || !(opt->Pr > 0) || !(opt->deltaT > 0) || opt->tauModel < 0 || opt->tauModel > 3)
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_create: rho0, Pr, deltaT must be positive, tauModel in 0..3");
    if ((opt->fluxSchemeU != QGD_FLUX_LINEAR && opt->fluxSchemeU != QGD_FLUX_UPWIND) || (opt->fluxSchemeT != QGD_FLUX_LINEAR && opt->fluxSchemeT != QGD_FLUX_UPWIND))
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_create: fluxSchemeU / fluxSchemeT must be QGD_FLUX_LINEAR or QGD_FLUX_UPWIND");
    int st = 0;
    const int rc = caseCreatePreamble("qgd_qhd_case_create", d, opt->stencil, &st);
    if (rc) return rc;
    qgd_qhd_case_s* c = new qgd_qhd_case_s();
    try {
        caseCoreInit(c, d, st);
        c->opt = *opt;
        d->ensureFaceGeoPos();
        const MeshView& v = d->view;
        if (!d->sharded() && opt->pRefCell >= v.nC) return caseAbandon(c, fail(QGD_ERR_INVALID, "qgd_qhd_case_create: pRefCell out of range"));
        DeviceArena& a = c->arena;
        QhdView& q = c->view;
        const size_t nC = (size_t)v.nC, nB = (size_t)std::max(v.nBF, 1), nF = (size_t)v.nF, nP = (size_t)std::max(v.nP, 1);
        q.c4 = a.alloc<double>(4 * nC); q.b4 = a.alloc<double>(4 * nB); q.pt4 = a.alloc<double>(4 * nP);
        q.p = a.alloc<double>(nC); q.pb = a.alloc<double>(nB); q.pgb = a.alloc<double>(nB); q.ptp = a.alloc<double>(nP);
        c->tauF = a.alloc<double>(nF); c->tbr = a.alloc<double>(nF); q.tauF = c->tauF;
        q.phiu = a.alloc<double>(nF); q.phiwo = a.alloc<double>(nF); q.phi = a.alloc<double>(nF); q.phitr = a.alloc<double>(nF);
        q.ugu = a.alloc<double>(3 * nF); q.gUc = a.alloc<double>(9 * nC); q.F = a.alloc<double>(4 * nF);
        c->scratch = a.alloc<double>(8);
        c->lagrange = envOnOff("QGD_QHD_LAGRANGE", 1) != 0;
        q.implicit = opt->implicitDiffusion ? 1 : 0;
        q.upwindU = opt->fluxSchemeU == QGD_FLUX_UPWIND ? 1 : 0;
        q.upwindT = opt->fluxSchemeT == QGD_FLUX_UPWIND ? 1 : 0;
        // (off by default: measured at 8 M cells the one launch takes what the three kernels take -- profiles/r06_ab_qhd_fused_advance.txt)
        if (envOnOff("QGD_QHD_FUSED", 0) != 0 && qhdFusedAdvanceEligible(st, v, q, nullptr, nullptr)) c->c4b = a.alloc<double>(4 * nC);
        if (q.implicit) {
            q.aG = a.alloc<double>(nF); q.diag4 = a.alloc<double>(4 * nC); q.rhs4 = a.alloc<double>(4 * nC); q.x4 = a.alloc<double>(4 * nC);
            c->implSolver = implicitSolverCreate(d->stream, v, d->ownedBegin, d->ownedEnd);
            c->implMask = 8;
            for (int k = 0; k < 3; ++k) if (!(v.nGeomD < 3 && v.emptyDir[k])) c->implMask |= 1 << k;   // validComponents (L0)
            {   // start values of the four systems: 0 = the current fields (OpenFOAM's), 1..3 = + the extrapolated time increment
                static const int kOrders[] = {0, 1, 2, 3, 4};
                c->implXOrder = envChoice("QGD_IMPL_XEXTRAP", 3, kOrders, 5);
                for (int j = 0; j < c->implXOrder; ++j) q.xd[j] = a.alloc<double>(4 * nC);
                q.xHave = 0; q.xOrder = c->implXOrder;
            }
        }
        q.rho0 = opt->rho0; q.nu = opt->mu / opt->rho0; q.Hi = (opt->mu / opt->Pr) / opt->rho0; q.beta = opt->beta;
        for (int k = 0; k < 3; ++k) q.g[k] = opt->g[k];
        q.dt = opt->deltaT; q.tauModel = opt->tauModel; q.Tau = opt->Tau; q.aQGD = opt->aQGD; q.UQHD = opt->UQHD; q.T0 = opt->T0; q.Gr = opt->Gr;
        c->bcPRequested.assign(d->patches.size(), QGD_BC_ZEROGRADIENT);
        casePatchTable(c);
        c->bKind = a.alloc<uint8_t>(nB);
        {
            static const int kModes[] = {0, 1, 2, 3, 4};
            c->pOrder = envChoice("QGD_QHD_PEXTRAP", 4, kModes, 5);   // 0: OpenFOAM's start value p^n; k: extrapolation of order k in time (qgd_qhd.hip)
            for (int j = 0; j < c->pOrder; ++j) c->pHist[j] = a.alloc<double>(nC);
        }
    } catch (...) { caseAbandon(c, 0); throw; }
    caseCount(c);
    *out = c;
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_free(qgd_qhd_case_t c) {
    if (!c) return QGD_OK;
    (void)hipSetDevice(c->dev->deviceId);
    if (c->solver) pressureSolverFree(c->solver);
    if (c->redHost) (void)hipHostFree(c->redHost);
    return caseAbandon(c, QGD_OK);
}
// QhdView::bValU follows the patches' flags: without a list the kernels read nothing (nullptr) and keep their list-free instantiations
static void qhdBcValuePointer(qgd_qhd_case_s* c) {
    int32_t any = 0;
    for (const PatchBCDev& b : c->bc) any |= b.valList;
    c->view.bValU = (any & QGD_BC_LIST_U) ? c->bValUDev : nullptr;
}
int qgd_qhd_case_set_bc(qgd_qhd_case_t c, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT, int32_t bcP,
                        double valueP) {
    QGD_TRY
    const int rc = casePatchEntry(c, "qgd_qhd_case_set_bc", patch, bcU, valueU, bcT, valueT, 2, bcP, valueP);
    if (rc) return rc;
    c->bcPRequested[patch] = bcP;
    qhdBcValuePointer(c);
    return QGD_OK;
    QGD_CATCH
}
// one velocity per face of a fixedValue patch: the contract of qgd_case_set_bc_values
int qgd_qhd_case_set_bc_values(qgd_qhd_case_t c, int32_t patch, const double* U, int64_t nFaces) {
    QGD_TRY
    int rc = bcValuesCheck(c, "qgd_qhd_case_set_bc_values", patch, 0, nFaces, U != nullptr,
                           "' is a halo, cyclic or constraint patch: its faces carry no fixedValue entry");
    if (rc == QGD_OK) rc = bcValuesStore(c, "qgd_qhd_case_set_bc_values", patch, 0, U, true, c->bValUDev, nullptr);
    if (rc) return rc;
    qhdBcValuePointer(c);
    return QGD_OK;
    QGD_CATCH
}
// SRFQHDFoam: the rotating frame's angular velocity and whether the T equation stays in the loop
int qgd_qhd_case_set_srf(qgd_qhd_case_t c, const double omega[3], int32_t flags) {
    QGD_TRY
    if (!c || !omega) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: null argument");
    if (c->solver) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: call it after qgd_qhd_case_create and before qgd_qhd_case_set_fields");
    if (flags & ~QGD_SRF_SOLVE_T) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: unknown flag bits");
    const qgd_device_s* d = c->dev;
    if (d->sharded())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_case_set_srf: a sharded device is not served (the rotating-frame case runs on one device's whole mesh)");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(omega[k])) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: non-finite omega");
    const MeshView& v = d->view;
    if (v.nGeomD < 2) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: a 1-D mesh has no plane for the Coriolis force to act in");
    if (v.nGeomD == 2)
        for (int k = 0; k < 3; ++k)
            if (!v.emptyDir[k] && omega[k] != 0.0)
                return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_srf: on a mesh with an empty direction omega must be parallel to it (the force's component along "
                                             "the empty direction is not solved for and would be dropped)");
    QhdView& q = c->view;
    for (int k = 0; k < 3; ++k) q.omega[k] = omega[k];
    q.rotating = (omega[0] != 0.0 || omega[1] != 0.0 || omega[2] != 0.0) ? 1 : 0;
    q.frozenT = (flags & QGD_SRF_SOLVE_T) ? 0 : 1;
    if (q.implicit) c->implMask = (c->implMask & 7) | (q.frozenT ? 0 : 8);   // frozen T: its system is not solved
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_srf_info(qgd_qhd_case_t c, double info[8]) {
    if (!c || !info) return fail(QGD_ERR_INVALID, "qgd_qhd_case_srf_info: null argument");
    for (int k = 0; k < 8; ++k) info[k] = 0.0;
    for (int k = 0; k < 3; ++k) info[k] = c->view.omega[k];
    info[3] = c->view.rotating; info[4] = c->view.frozenT;
    return QGD_OK;
}
int qgd_qhd_case_set_fields(qgd_qhd_case_t c, const double* U, const double* T, const double* p) {
    QGD_TRY
    if (!c || !U || !T || !p) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_fields: null argument");
    qgd_device_s* d = c->dev;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& m = d->view;
    if (!c->bc.empty()) HIP_CHECK(hipMemcpy(c->bcDev, c->bc.data(), sizeof(PatchBCDev) * c->bc.size(), hipMemcpyHostToDevice));
    // matrix kinds of the pressure equation per boundary face; fvMatrix::setReference acts only without a fixedValue patch
    std::vector<uint8_t> kind((size_t)std::max(m.nBF, 1), 0);
    bool anyFixed = false;
    for (size_t ip = 0; ip < d->patches.size(); ++ip) {
        const Patch& pt = d->patches[ip];
        int k = c->bc[ip].bcP;
        if (pt.type != QGD_PATCH_GENERIC) k = QGD_BC_NONE;
        const uint8_t kk = k == QGD_BC_FIXEDVALUE ? 1 : ((k == QGD_BC_QGDFLUX || k == QGD_BC_QHDFLUX) ? 2 : 0);
        // "does p need a reference level" is a property of the WHOLE mesh: a fixedValue patch counts when it has faces anywhere
        // (a shard may hold none of them; on an inner box slab the patch is the cut plane and only the caller's request is known)
        const bool genericGlobally = pt.type == QGD_PATCH_GENERIC || (pt.type == QGD_PATCH_HALO && pt.globalSize >= 0 && d->cellGlobal.empty());
        if (c->bcPRequested[ip] == QGD_BC_FIXEDVALUE && genericGlobally && pt.nonEmptyGlobally()) anyFixed = true;
        for (int32_t f = pt.start; f < pt.start + pt.size; ++f) kind[(size_t)(f - m.nIF)] = kk;
    }
    HIP_CHECK(hipMemcpy(c->bKind, kind.data(), kind.size(), hipMemcpyHostToDevice));
    c->needRef = !anyFixed && c->opt.pRefCell >= 0;
    c->localRefCell = c->needRef ? (d->sharded() ? d->ownedLocalOf(c->opt.pRefCell) : c->opt.pRefCell) : -1;
    Workspace& ws = d->ws;
    double* dU = ws.get<double>(WS_CELL, 3 * (size_t)m.nC);
    double* dT = ws.get<double>(WS_A, (size_t)m.nC);
    double* dp = ws.get<double>(WS_B, (size_t)m.nC);
    ws.h2d(dU, U, sizeof(double) * 3 * (size_t)m.nC, d->stream);
    ws.h2d(dT, T, sizeof(double) * (size_t)m.nC, d->stream);
    ws.h2d(dp, p, sizeof(double) * (size_t)m.nC, d->stream);
    (void)hipGetLastError();
    HIP_CHECK(hipMemsetAsync(c->view.phiwo, 0, sizeof(double) * (size_t)m.nF, d->stream));
    launchQhdInit(d->stream, m, c->view, c->bcDev, dU, dT, dp, c->tauF, c->tbr);
    c->view.dt = c->opt.deltaT;   // (an adjusted run before this call may have left another)
    if (c->view.implicit) {   // the matrix of the U and T equations: constant in time up to V/deltaT on the diagonals (thermo is not corrected in the loop)
        launchQhdImplicitMatrix(d->stream, m, c->view, c->bcDev);
        c->dtDiag = c->view.dt;
        implicitStatsReset(c->implSolver);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(d->stream));
    c->tcReady = false; c->minTau = 0; c->maxUh = 0; c->CoNum = 0; c->coSteps = -1;
    c->dtHist.clear();
    if (c->solver) { pressureSolverFree(c->solver); c->solver = nullptr; }
    c->solver = pressureSolverCreate(d->stream, m, c->tbr, c->bKind, c->localRefCell, c->opt.precond, d->ownedBegin, d->ownedEnd,
                                     d->cellGlobal.empty() ? nullptr : d->cellGlobal.data(), d->cellGlobalOffset, d->sharded());
    c->fieldsSet = true;
    c->pPrevHave = 0;
    c->view.xHave = 0;
    c->time = 0; c->steps = 0;
    return QGD_OK;
    QGD_CATCH
}
// One step as stream-ordered phases (the exchanges of a sharded run go between them, see include/qgd_amd.h):
//   0 flux assembly + rhs + first residual | 1 normFactor | 2 first preconditioned residual | 3, 4, 5 one PCG iteration |
//   6 p's boundary conditions after the solve | 7 phi, the U and T equations | 8 reference level of p
static void qhdPhase(qgd_qhd_case_s* c, int phase) {
    qgd_device_s* d = c->dev;
    const MeshView& m = d->view;
    (void)hipGetLastError();
    switch (phase) {
        case 0:
            launchQhdAssemble(d->stream, c->stencil, c->usesPoints, m, c->view, c->bcDev);
            if (c->pOrder > 0) {
                // p of this solve belongs to the state the last step left: one step of the last deltaT ahead of the p before it
                QhdStartWeights W;
                const int k = std::min(c->pPrevHave, c->pOrder);
                if (!c->dtHist.empty() && qhdStartWeights(c, c->dtHist[0], 1, k, W)) launchQhdExtrapolatePW(d->stream, m.nC, c->view.p, c->pHist, c->pOrder, W);
                else launchQhdExtrapolateP(d->stream, m.nC, c->view.p, c->pHist, c->pPrevHave, c->pOrder);
                c->pPrevHave = std::min(c->pPrevHave + 1, c->pOrder);
            }
            pressureSolveBegin(c->solver, c->view.phiu, c->view.phiwo, c->view.pb, c->view.pgb, c->opt.pTol, c->opt.pRelTol, c->opt.pMaxIter, c->view.p);
            break;
        case 1: case 2: case 3: case 4: case 5: pressureSolvePhase(c->solver, phase); break;
        case 6: launchQhdPostSolve(d->stream, m, c->view, c->bcDev); break;
        case 7:
            pressureSolveFlux(c->solver, c->view.phi);
            // (adjustTimeStep, or its end: the diagonals follow deltaT -- the dtDiag pattern of the scalar case)
            if (c->view.implicit && c->view.dt != c->dtDiag) { launchQhdImplicitDiag(d->stream, m, c->view, c->bcDev); c->dtDiag = c->view.dt; }
            if (!c->view.implicit)
            {
                if (launchQhdAdvance(d->stream, c->stencil, c->usesPoints, m, c->view, c->bcDev, c->needRef, c->localRefCell, c->opt.pRefValue,
                                     pressureSolverCtl(c->solver) + 8, c->c4b))
                    std::swap(c->view.c4, c->c4b);   // the blocks wrote the new {U,T} into the second array
            } else {
                // implicitDiffusion: face pass 2 without the laplacians, the right-hand sides; the solve (phases 10..15) and phase 16 follow
                implicitStepMark(c->implSolver, true);
                {
                    // the start values one step of the NEW deltaT ahead of the current fields; under unequal steps with the weights by value
                    QhdStartWeights W;
                    const bool byValue = c->view.xOrder > 0 && qhdStartWeights(c, c->view.dt, 0, std::min(c->view.xHave, c->view.xOrder), W);
                    QhdView qv = c->view;
                    if (byValue) qv.xOrder = 0;
                    launchQhdImplicitAdvance(d->stream, c->stencil, c->usesPoints, m, qv, c->bcDev, 0, c->implMask, false, -1, 0.0, nullptr);
                    if (byValue) launchQhdStartValuesW(d->stream, m, c->view, W);
                }
                if (c->view.xOrder > 0) {   // the right-hand-side kernel put the current fields into the oldest slot: it becomes the newest
                    QhdView& q = c->view;
                    double* t = q.xd[q.xOrder - 1];
                    for (int j = q.xOrder - 1; j >= 1; --j) q.xd[j] = q.xd[j - 1];
                    q.xd[0] = t;
                    q.xHave = std::min(q.xHave + 1, q.xOrder);
                }
                const double gamma[4] = {c->view.nu, c->view.nu, c->view.nu, c->view.Hi};
                // (frozen T, SRFQHDFoam: the three U systems alone -- the first three planes of the component-major vectors)
                implicitSolveSetup(c->implSolver, c->view.frozenT ? 3 : 4, c->implMask, c->view.aG, c->view.diag4, c->view.rhs4, c->view.x4,
                                   c->opt.implicitTol, c->opt.implicitMaxIter, gamma);
            }
            break;
        case 10: case 11: case 12: case 13: case 14: case 15:
            if (!c->view.implicit) throw std::invalid_argument("qgd_qhd_case_step_phase: phases 10..16 belong to the implicitDiffusion branch");
            implicitSolvePhase(c->implSolver, phase - 10);
            break;
        case 16:
            if (!c->view.implicit) throw std::invalid_argument("qgd_qhd_case_step_phase: phases 10..16 belong to the implicitDiffusion branch");
            implicitSolveEnd(c->implSolver, 0);
            implicitStepMark(c->implSolver, false);
            launchQhdImplicitAdvance(d->stream, c->stencil, c->usesPoints, m, c->view, c->bcDev, 1, c->implMask, c->needRef, c->localRefCell,
                                     c->opt.pRefValue, pressureSolverCtl(c->solver) + 8);
            break;
        case 8:
            launchQhdFinish(d->stream, m, c->view, c->needRef, pressureSolverCtl(c->solver) + 8);
            c->time += c->view.dt;   // (the options' deltaT, or the one the step's control set)
            c->steps++;
            c->dtHist.insert(c->dtHist.begin(), c->view.dt);
            if (c->dtHist.size() > 6) c->dtHist.pop_back();
            break;
        case 9: pressureSolveContinue(c->solver); break;   // after the collective qgd_qhd_case_pending asked for
        default: throw std::invalid_argument("qgd_qhd_case_step_phase: phase must be 0..9 (10..16: implicitDiffusion)");
    }
    HIP_CHECK(hipGetLastError());
}
static void qhdReadStatus(qgd_qhd_case_s* c) {
    double st[4];
    pressureSolveStatus(c->solver, st);
    c->lastIter = st[1]; c->lastRes0 = st[2]; c->lastRes = st[3];
}
// a whole step with the transport behind `hooks` (nullptr: one rank); haloState(kind) exchanges message kind 0 or 1
static void qhdStepWith(qgd_qhd_case_s* c, const SolveHooks* hooks, const std::function<void(int)>& haloState) {
    if (c->adjust) qhdTimeControlReady(c);
    qhdPhase(c, 0);
    if (c->adjust) qhdCourantQueue(c);                 // QHDCourantNo.H: after updateFluxes.H [QHDFoam.C L102-105]
    HIP_CHECK(hipStreamSynchronize(c->dev->stream));   // one wait per step, so that lastSolveMs is the solve alone
    if (c->adjust) qhdSetDeltaT(c);                    // setDeltaT-QGDQHD.H [L106]; the pressure equation does not hold deltaT, phase 7 does
    const double t0 = nowMs();
    double res[2];
    c->lastIter = pressureSolveRun(c->solver, hooks, res);
    c->lastRes0 = res[0]; c->lastRes = res[1];
    c->lastSolveMs = nowMs() - t0;
    qhdPhase(c, 6);
    if (haloState) haloState(1);
    qhdPhase(c, 7);
    if (c->view.implicit) {
        // the four systems of QHDUEqn.H L48-64 / QHDTEqn.H L71-79 as one solve; on shards its reductions and the ghost entries of
        // the iterate go through the hooks (message kind 4)
        SolveHooks ih;
        if (hooks) { ih.allreduce = hooks->allreduce; ih.allreduceBuf = hooks->allreduceBuf; }
        if (haloState) ih.haloDirection = [&]() { haloState(4); };
        implicitSolveRun(c->implSolver, &ih);
        qhdPhase(c, 16);
    }
    if (c->needRef && hooks && hooks->allreduce) hooks->allreduce(pressureSolverCtl(c->solver) + 8, 1);
    qhdPhase(c, 8);
    if (haloState) haloState(0);
}
int qgd_qhd_case_step(qgd_qhd_case_t c, int32_t nSteps) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_qhd_case_step: call qgd_qhd_case_set_fields first");
    qgd_device_s* d = c->dev;
    if (d->sharded())
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_step: sharded mesh, drive it with qgd_qhd_case_step_phase + the exchanges, or qgd_qhd_case_step_sharded");
    HIP_CHECK(hipSetDevice(d->deviceId));
    for (int i = 0; i < nSteps; ++i) qhdStepWith(c, nullptr, nullptr);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_step_phase(qgd_qhd_case_t c, int phase) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_qhd_case_step_phase: call qgd_qhd_case_set_fields first");
    if (phase < 0 || phase > 16) return fail(QGD_ERR_INVALID, "qgd_qhd_case_step_phase: phase must be 0..9 (10..16: implicitDiffusion)");
    if (c->adjust) return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_case_step_phase: adjustTimeStep (qgd_qhd_case_set_time_control) is served by qgd_qhd_case_step alone");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    qhdPhase(c, phase);
    return QGD_OK;   // stream-ordered: qgd_qhd_case_solve_status / qgd_qhd_case_sync wait
    QGD_CATCH
}
int qgd_qhd_case_control_ptr(qgd_qhd_case_t c, void** devicePtr) {
    if (!c || !devicePtr) return fail(QGD_ERR_INVALID, "null argument");
    if (!c->solver) return fail(QGD_ERR_INVALID, "qgd_qhd_case_control_ptr: call qgd_qhd_case_set_fields first");
    *devicePtr = pressureSolverCtl(c->solver);
    return QGD_OK;
}
int qgd_qhd_case_sweep_time(qgd_qhd_case_t c, int reps, double info[4]) {
    QGD_TRY
    if (!c || !info || reps <= 0) return fail(QGD_ERR_INVALID, "bad argument");
    if (!c->solver) return fail(QGD_ERR_INVALID, "qgd_qhd_case_sweep_time: call qgd_qhd_case_set_fields first");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    int rows = 0;
    double width = 0;
    info[0] = pressureSolverSweepMs(c->solver, reps, &rows, &width);
    info[1] = rows; info[2] = width; info[3] = pressureSolverSinglePrecisionCycle(c->solver) ? 4.0 : 8.0;
    return QGD_OK;
    QGD_CATCH
}
// the three read-only entries on the pressure preconditioner: 0 when the cycle is observable, else the status (last error set)
static int qhdMgRefused(qgd_qhd_case_t c, const char* who) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->solver) return fail(QGD_ERR_INVALID, std::string(who) + ": call qgd_qhd_case_set_fields first");
    if (c->dev->sharded() || !pressureSolverMgObservable(c->solver))
        return fail(QGD_ERR_NOT_IMPLEMENTED, std::string(who) + ": the multigrid cycle of an unsharded case with precond = 1 only");
    return QGD_OK;
}
int qgd_qhd_case_mg_info(qgd_qhd_case_t c, double* info, int32_t cap) {
    QGD_TRY
    if (const int rc = qhdMgRefused(c, "qgd_qhd_case_mg_info")) return rc;
    if (!info || cap < 1) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_info: bad argument");
    const int need = pressureSolverMgInfo(c->solver, info, cap);
    if (need > cap) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_info: info needs " + std::to_string(need) + " doubles");
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_mg_get(qgd_qhd_case_t c, int32_t level, int32_t what, void* buf, int64_t cap, int64_t* n) {
    QGD_TRY
    if (const int rc = qhdMgRefused(c, "qgd_qhd_case_mg_get")) return rc;
    if (!n) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_get: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const int64_t count = pressureSolverMgGet(c->solver, level, what, nullptr, 0);
    if (count < 0) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_get: no such level or array");
    *n = count;
    if (!buf) return QGD_OK;
    if (cap < count) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_get: buf holds " + std::to_string(cap) + " of " + std::to_string(count) + " elements");
    pressureSolverMgGet(c->solver, level, what, buf, cap);
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_mg_apply(qgd_qhd_case_t c, const double* r, double* z, int32_t mode, double* rzPart) {
    QGD_TRY
    if (const int rc = qhdMgRefused(c, "qgd_qhd_case_mg_apply")) return rc;
    if (!r || !z || mode < 0 || mode > 1 || (mode == 1 && !rzPart)) return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_apply: bad argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    if (!pressureSolverMgApply(c->solver, r, z, mode == 1, rzPart))
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_mg_apply: mode 1 needs the fused hand-over of a single-precision cycle (QGD_MG_F32, QGD_MG_FUSE)");
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_control(qgd_qhd_case_t c, double control[16], int set) {
    QGD_TRY
    if (!c || !control) return fail(QGD_ERR_INVALID, "null argument");
    if (!c->solver) return fail(QGD_ERR_INVALID, "qgd_qhd_case_control: call qgd_qhd_case_set_fields first");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    hipStream_t st = c->dev->stream;
    if (set) HIP_CHECK(hipMemcpyAsync(pressureSolverCtl(c->solver), control, 16 * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_CHECK(hipMemcpyAsync(control, pressureSolverCtl(c->solver), 16 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return QGD_OK;
    QGD_CATCH
}
// ---- the accessors of the implicitDiffusion solve, of a QGD and of a QHD case: `refusal` is the entry's text for a null argument or a case
// without the branch.  The control block (68 doubles, slot-major: control[slot * 4 + component]) and the state of the solve in flight
static int caseImplicitControl(CaseCore* c, const char* refusal, double* control, int set) {
    QGD_TRY
    if (!c || !control || !c->implSolver) return fail(QGD_ERR_INVALID, refusal);
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    hipStream_t st = c->stream();
    if (set) HIP_CHECK(hipMemcpyAsync(implicitSolverCtl(c->implSolver), control, 68 * sizeof(double), hipMemcpyHostToDevice, st));
    else HIP_CHECK(hipMemcpyAsync(control, implicitSolverCtl(c->implSolver), 68 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return QGD_OK;
    QGD_CATCH
}
static int caseImplicitControlPtr(CaseCore* c, const char* refusal, void** devicePtr) {
    if (!c || !devicePtr || !c->implSolver) return fail(QGD_ERR_INVALID, refusal);
    *devicePtr = implicitSolverCtl(c->implSolver);
    return QGD_OK;
}
// status: {all components done, right-hand sides of the solve in flight}; maxRhs: 3 (a QGD case's solves) or 4 (the QHD case's) are read
static int caseImplicitSolveStatus(CaseCore* c, const char* refusal, int maxRhs, double status[2]) {
    QGD_TRY
    if (!c || !status || !c->implSolver) return fail(QGD_ERR_INVALID, refusal);
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    implicitSolverSetStream(c->implSolver, c->stream());
    int it[4];
    double r0[4], r1[4];
    if (maxRhs == 3) implicitSolveStatus(c->implSolver, &status[0], it, r0, r1);
    else implicitSolveStatus4(c->implSolver, &status[0], it, r0, r1);
    status[1] = implicitSolverRhs(c->implSolver);
    return QGD_OK;
    QGD_CATCH
}
// info: iterations [0..4), initial [4..8) and final residuals [8..12) of four systems, [12] steps with a solve above its tolerance, [13] the
// algorithm (0: no branch, 1: conjugate gradients (QGD_IMPL_SOLVER=pcg), 2: Chebyshev iteration), [14] stalled steps.  lastStep: the systems
// are Ux, Uy, Uz, e of the QGD case's two solves as the last step left them, else the four of the QHD case's one solve as it stands
static int caseImplicitInfo(CaseCore* c, const char* refusal, bool lastStep, double info[16]) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, refusal);
    for (int k = 0; k < 16; ++k) info[k] = 0.0;
    ImplicitSolver* S = c->implSolver;
    if (!S) return QGD_OK;
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    implicitSolverSetStream(S, c->stream());
    int it[4];
    double r0[4], r1[4], bad = 0, stalled = 0;
    if (lastStep) implicitSolverInfo(S, it, r0, r1, &bad, &stalled);
    else {
        double allDone = 0;
        implicitSolveStatus4(S, &allDone, it, r0, r1);
        bad = implicitSolverUnconverged(S, &stalled);
    }
    for (int k = 0; k < 4; ++k) { info[k] = it[k]; info[4 + k] = r0[k]; info[8 + k] = r1[k]; }
    info[12] = bad; info[13] = implicitSolverChebyshev(S) ? 2.0 : 1.0; info[14] = stalled;
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_implicit_control(qgd_qhd_case_t c, double control[68], int set) {
    return caseImplicitControl(c, "qgd_qhd_case_implicit_control: an implicitDiffusion case is needed", control, set);
}
int qgd_qhd_case_implicit_control_ptr(qgd_qhd_case_t c, void** devicePtr) {
    return caseImplicitControlPtr(c, "qgd_qhd_case_implicit_control_ptr: an implicitDiffusion case is needed", devicePtr);
}
int qgd_qhd_case_implicit_info(qgd_qhd_case_t c, double info[16]) { return caseImplicitInfo(c, "bad argument", false, info); }
int qgd_qhd_case_implicit_solve_status(qgd_qhd_case_t c, double status[2]) {
    return caseImplicitSolveStatus(c, "qgd_qhd_case_implicit_solve_status: an implicitDiffusion case is needed", 4, status);
}
int qgd_qhd_case_solve_status(qgd_qhd_case_t c, double status[4]) {
    QGD_TRY
    if (!c || !status) return fail(QGD_ERR_INVALID, "null argument");
    if (!c->solver) return fail(QGD_ERR_INVALID, "qgd_qhd_case_solve_status: call qgd_qhd_case_set_fields first");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    pressureSolveStatus(c->solver, status);
    c->lastIter = status[1]; c->lastRes0 = status[2]; c->lastRes = status[3];
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_sync(qgd_qhd_case_t c) { return caseSync(c); }
// what the phase in flight waits for before qgd_qhd_case_step_phase(c, 9): see include/qgd_amd.h
int qgd_qhd_case_pending(qgd_qhd_case_t c, int32_t* action, void** devicePtr, int64_t* count) {
    if (!c || !action) return fail(QGD_ERR_INVALID, "bad argument");
    double* buf = nullptr;
    int64_t n = 0;
    *action = c->solver ? pressureSolvePending(c->solver, &buf, &n) : 0;
    if (devicePtr) *devicePtr = buf;
    if (count) *count = n;
    return QGD_OK;
}
// ---- the halo messages of the QHD case: kind 0 (state), 1 (p), 2 (search direction), 3 (the iterate of the multigrid level that spans the
// ranks), 4 (the iterate of the implicit solve, {Ux, Uy, Uz, T}) ------------------------------------------------------------------------
static int caseHaloMove(qgd_qhd_case_s* c, int slot, int kind, double* buf, bool pack, hipStream_t stream) {
    qgd_device_s* d = c->dev;
    if (slot >= (int)d->halo.size()) return QGD_OK;
    const qgd_device_s::HaloSlot& h = d->halo[slot];
    const int32_t nCells = pack ? h.nSend : h.nGhost, nFaces = pack ? h.nSendBF : h.nGhostBF;
    if (nCells + nFaces == 0) return QGD_OK;
    if (!buf) return fail(QGD_ERR_INVALID, "null buffer");
    if (kind >= 2 && !c->solver) return fail(QGD_ERR_INVALID, "no solve in flight");
    if (kind == 4 && !c->implSolver) return fail(QGD_ERR_INVALID, "message kind 4 belongs to the implicitDiffusion branch");
    float* vec = kind == 3 ? pressureSolverMgHaloVec(c->solver) : nullptr;
    if (kind == 3 && !vec) return fail(QGD_ERR_INVALID, "message kind 3: no multigrid iterate is waiting for its ghost entries (qgd_qhd_case_pending)");
    (void)hipGetLastError();   // a stale error of an earlier, refused call must not be taken for this launch's
    if (kind == 4) launchSolverHalo(stream, c->implSolver, pack ? h.send : h.ghost, nCells, buf, pack);
    else if (kind == 3) launchQhdHaloFloat(stream, vec, pack ? h.send : h.ghost, nCells, buf, pack);
    else launchQhdHalo(stream, c->view, c->solver ? pressureSolverDirection(c->solver) : nullptr, kind, pack ? h.send : h.ghost, nCells,
                       pack ? h.sendBF : h.ghostBF, nFaces, buf, pack);
    HIP_CHECK(hipGetLastError());
    return QGD_OK;
}
static HaloMessage haloMessage(qgd_qhd_case_s* c, int kind) {
    HaloMessage m;
    m.perCell = kind == 0 ? 4 : (kind == 1 ? 10 : (kind == 4 ? 4 : 1));
    m.perFace = kind == 0 ? 4 : (kind == 1 ? 2 : 0);
    m.move = [c, kind](int slot, double* buf, bool pack, hipStream_t stream) { return caseHaloMove(c, slot, kind, buf, pack, stream); };
    return m;
}
static HaloBuffers& haloBuffers(qgd_qhd_case_s* c) {
    c->haloBuf.arena = &c->arena;
    c->haloBuf.widest.perCell = 10;   // p
    c->haloBuf.widest.perFace = 4;    // state
    return c->haloBuf;
}
int qgd_qhd_case_halo_count(qgd_qhd_case_t c, int slot, int kind, int64_t* sendCount, int64_t* recvCount) {
    if (!c || slot < 0 || kind < 0 || kind > 4 || !sendCount || !recvCount) return fail(QGD_ERR_INVALID, "bad argument");
    return caseHaloCount(c, slot, haloMessage(c, kind), sendCount, recvCount);
}
int qgd_qhd_case_halo_pack(qgd_qhd_case_t c, int slot, int kind, double* sendBufDevice) {
    if (!c || slot < 0 || kind < 0 || kind > 4) return fail(QGD_ERR_INVALID, "bad argument");
    return caseHaloMovePublic(c, slot, haloMessage(c, kind), sendBufDevice, true, c->stream());
}
int qgd_qhd_case_halo_unpack(qgd_qhd_case_t c, int slot, int kind, const double* recvBufDevice) {
    if (!c || slot < 0 || kind < 0 || kind > 4) return fail(QGD_ERR_INVALID, "bad argument");
    return caseHaloMovePublic(c, slot, haloMessage(c, kind), recvBufDevice, false, c->stream());
}
int qgd_qhd_case_get_field(qgd_qhd_case_t c, const char* name, double* out, int64_t outDoubles) {
    QGD_TRY
    if (!c || !name || !out) return fail(QGD_ERR_INVALID, "qgd_qhd_case_get_field: null argument");
    qgd_device_s* d = c->dev;
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    const MeshView& m = d->view;
    std::string s(name);
    const bool bnd = boundaryName(s);
    const int64_t n = bnd ? m.nBF : m.nC;
    const QhdView& q = c->view;
    const double* direct = nullptr;
    int64_t count = 0;
    if (s == "p") { direct = bnd ? q.pb : q.p; count = n; }
    else if (!bnd && s == "phi") { direct = q.phi; count = m.nF; }
    else if (!bnd && s == "phiu") { direct = q.phiu; count = m.nF; }
    else if (!bnd && s == "phiwo") { direct = q.phiwo; count = m.nF; }
    else if (!bnd && s == "tauQGDf") { direct = c->tauF; count = m.nF; }
    else if (!bnd && s == "hQGDf") { direct = m.hf; count = m.nF; }
    else if (!bnd && s == "faceTerms") {
        // QhdView::F by face label: the four net face terms of the U (3) and T equations, component-major (an internal face keeps its
        // terms at its slot-major position MeshView::fpos, a patch face at its label); under implicitDiffusion the explicit part
        if (c->steps == 0) return fail(QGD_ERR_INVALID, "qgd_qhd_case_get_field: faceTerms hold nothing before the first step after qgd_qhd_case_set_fields");
        const size_t nF = (size_t)m.nF;
        if ((int64_t)(4 * nF) > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        std::vector<double> F(4 * nF);
        std::vector<int32_t> fpos((size_t)m.nIF);
        if (nF) HIP_CHECK(hipMemcpy(F.data(), q.F, sizeof(double) * 4 * nF, hipMemcpyDeviceToHost));
        if (m.nIF) HIP_CHECK(hipMemcpy(fpos.data(), m.fpos, sizeof(int32_t) * (size_t)m.nIF, hipMemcpyDeviceToHost));
        for (int k = 0; k < 4; ++k)
            for (size_t f = 0; f < nF; ++f) out[(size_t)k * nF + f] = F[(size_t)k * nF + (f < (size_t)m.nIF ? (size_t)fpos[f] : f)];
        return QGD_OK;
    }
    if (direct) {
        if (count > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        if (count) d->ws.d2h(out, direct, sizeof(double) * (size_t)count, d->stream);
        return QGD_OK;
    }
    if (s != "U" && s != "T") return fail(QGD_ERR_UNKNOWN_NAME, "qgd_qhd_case_get_field: unknown field " + s);
    const int nc = s == "U" ? 3 : 1;
    if (n * nc > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
    if (n == 0) return QGD_OK;
    double* tmp = d->ws.get<double>(WS_OUT, (size_t)(n * nc));
    (void)hipGetLastError();
    launchQhdExtract(d->stream, n, bnd ? q.b4 : q.c4, s == "U" ? 0 : 1, tmp);
    HIP_CHECK(hipGetLastError());
    d->ws.d2h(out, tmp, sizeof(double) * (size_t)(n * nc), d->stream);
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_info(qgd_qhd_case_t c, double info[8]) {
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    int sizes[16];
    info[0] = c->time; info[1] = c->view.dt; info[2] = c->lastIter; info[3] = c->lastRes0; info[4] = c->lastRes; info[5] = (double)c->steps;
    info[6] = c->solver ? (double)pressureSolverLevels(c->solver, sizes, 16) : 0.0;
    info[7] = c->lastSolveMs;
    return QGD_OK;
}

// readTimeControls.H: the controls of QHDCourantNo.H / setDeltaT-QGDQHD.H, from the next step on
int qgd_qhd_case_set_time_control(qgd_qhd_case_t c, int32_t adjustTimeStep, double maxCo, double maxDeltaT, double cTau) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_time_control: null case");
    if (c->dev->sharded())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_case_set_time_control: a sharded device is not served (the Courant number would need a MAX all-reduce "
                                             "point in the phase table)");
    if (!(std::isfinite(maxCo) && maxCo > 0) || !(std::isfinite(maxDeltaT) && maxDeltaT > 0) || !(std::isfinite(cTau) && cTau > 0))
        return fail(QGD_ERR_INVALID, "qgd_qhd_case_set_time_control: maxCo, maxDeltaT, cTau must be finite and positive");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    c->adjust = adjustTimeStep != 0;
    c->maxCo = maxCo; c->maxDeltaT = maxDeltaT; c->cTau = cTau;
    if (!c->adjust) c->view.dt = c->opt.deltaT;   // (the diagonals of implicitDiffusion follow at the next step: dtDiag)
    return QGD_OK;
    QGD_CATCH
}
int qgd_qhd_case_time_info(qgd_qhd_case_t c, double info[8]) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, "qgd_qhd_case_time_info: null argument");
    if (!c->dev->sharded()) qhdTimeControlReady(c);
    if (c->fieldsSet && c->steps > 0 && c->coSteps != c->steps && !c->dev->sharded()) {
        // no control at the last step: its fluxes still stand in phiu (what QHDFoam.C L88-92 prints under a fixed deltaT)
        HIP_CHECK(hipSetDevice(c->dev->deviceId));
        qhdCourantQueue(c);
        HIP_CHECK(hipStreamSynchronize(c->dev->stream));
        c->maxUh = std::max(c->redHost[0], 0.0);
        c->CoNum = c->view.dt * c->maxUh;
        c->coSteps = c->steps;
    }
    const bool have = c->coSteps == c->steps && c->steps > 0;
    info[0] = c->time; info[1] = c->view.dt; info[2] = have ? c->CoNum : 0.0; info[3] = have ? c->maxUh : 0.0; info[4] = c->minTau;
    info[5] = c->adjust ? 1.0 : 0.0; info[6] = (double)c->steps; info[7] = 0.0;
    return QGD_OK;
    QGD_CATCH
}

int qgd_qhd_case_fused_info(qgd_qhd_case_t c, int64_t info[4]) {
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    info[0] = info[1] = info[2] = info[3] = 0;
    int lds = 0;
    if (c->c4b && qhdFusedAdvanceEligible(c->stencil, c->dev->view, c->view, &lds, nullptr)) { info[0] |= 1; info[1] = c->dev->view.fuBlocks; info[2] = lds; }
    return QGD_OK;
}

// ---- scalarTransportQHDFoam case resident on the device (qgd_scalar.hip) -------------------------------------------------
struct qgd_scalar_case_s : CaseCore {   // (implSolver: the T equation's one system)
    qgd_scalar_options opt{};
    ScalarView view{};
    double *work = nullptr, *red = nullptr;
    // the two extrema the time-step control reads are constants of the run (U, tauQGDf and the mesh do not change): reduced once on the
    // device at set_fields, the rule itself is then host arithmetic on them and no step waits for the device
    double maxUh = 0, minTau = 0;
    double dt = 0, dtDiag = 0, CoNum = 0;   // dtDiag: the deltaT view.diag was built with
};

int qgd_scalar_options_default(qgd_scalar_options* o) {
    if (!o) return fail(QGD_ERR_INVALID, "null argument");
    std::memset(o, 0, sizeof(*o));
    o->stencil = QGD_FVSC_GAUSSVOLPOINT;
    o->implicitDiffusion = 1; o->tauModel = 0; o->fluxSchemeT = QGD_FLUX_LINEAR; o->implicitMaxIter = 1000;
    o->rho0 = 1.0; o->mu = 0.0; o->Pr = 1.0; o->deltaT = 1e-3;
    o->Tau = 1e-3; o->aQGD = 0.5; o->UQHD = 1.0; o->T0 = 1.0; o->Gr = 1e3;
    o->maxCo = 0.5; o->maxDeltaT = 1e300; o->cTau = 0.75;
    o->implicitTol = 1e-10;
    return QGD_OK;
}
int qgd_scalar_case_create(qgd_device_t d, const qgd_scalar_options* opt, qgd_scalar_case_t* out) {
    QGD_TRY
    if (!d || !opt || !out) return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: null argument");
    if (d->periodic())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_scalar_case_create: a mesh whose cyclic patches were unrolled into ghost cells (qgd_mesh_unroll_cyclic) is "
                                             "not served: the implicit laplacian would need the coupled rows of the periodic pairs");
    if (d->sharded())
        return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_scalar_case_create: a sharded device is not served: the scalarTransportQHDFoam case runs on one device "
                                             "(no halo exchange of T, no reductions across shards)");
    if (!(opt->implicitTol > 0) || opt->implicitMaxIter < 1)
        return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: implicitTol must be positive, implicitMaxIter >= 1");
    if (!(opt->rho0 > 0) || !(opt->Pr > 0) || !(opt->deltaT > 0) || !(opt->mu >= 0) || opt->tauModel < 0 || opt->tauModel > 3)
        return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: rho0, Pr, deltaT must be positive, mu >= 0, tauModel in 0..3");
    if (opt->tauModel == 3 && !(opt->mu > 0)) return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: H2bynuQHD needs mu > 0");
    if (opt->fluxSchemeT != QGD_FLUX_LINEAR && opt->fluxSchemeT != QGD_FLUX_UPWIND)
        return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: fluxSchemeT must be QGD_FLUX_LINEAR or QGD_FLUX_UPWIND");
    if (opt->adjustTimeStep && (!(opt->maxCo > 0) || !(opt->maxDeltaT > 0) || !(opt->cTau > 0)))
        return fail(QGD_ERR_INVALID, "qgd_scalar_case_create: adjustTimeStep needs maxCo, maxDeltaT, cTau > 0");
    int st = 0;
    const int rc = caseCreatePreamble("qgd_scalar_case_create", d, opt->stencil, &st);
    if (rc) return rc;
    qgd_scalar_case_s* c = new qgd_scalar_case_s();
    try {
        caseCoreInit(c, d, st);
        c->opt = *opt;
        const MeshView& v = d->view;
        DeviceArena& a = c->arena;
        ScalarView& q = c->view;
        const size_t nC = (size_t)v.nC, nB = (size_t)std::max(v.nBF, 1), nF = (size_t)std::max(v.nF, 1), nP = (size_t)std::max(v.nP, 1);
        q.T = a.alloc<double>(nC); q.Tb = a.alloc<double>(nB); q.ptT = a.alloc<double>(c->usesPoints ? nP : 1);
        q.tauF = a.alloc<double>(nF); q.Uf = a.alloc<double>(3 * nF); q.phiu = a.alloc<double>(nF); q.tpu = a.alloc<double>(3 * nF); q.a = a.alloc<double>(nF);
        q.divPhiu = a.alloc<double>(nC); q.diagBase = a.alloc<double>(nC); q.srcB = a.alloc<double>(nC);
        q.F = a.alloc<double>(nF); q.diag = a.alloc<double>(nC); q.rhs = a.alloc<double>(nC);
        q.dbg = nullptr;
        c->work = a.alloc<double>(2 * ((nF + 255) / 256) + 2);   // two partials per workgroup of the set-up face kernel
        c->red = a.alloc<double>(2);
        q.Hi = (opt->mu / opt->Pr) / opt->rho0;
        q.upwindT = opt->fluxSchemeT == QGD_FLUX_UPWIND ? 1 : 0;
        q.tauModel = opt->tauModel; q.Tau = opt->Tau; q.aQGD = opt->aQGD; q.UQHD = opt->UQHD; q.T0 = opt->T0; q.Gr = opt->Gr; q.nu = opt->mu / opt->rho0;
        if (opt->implicitDiffusion) c->implSolver = implicitSolverCreate(d->stream, v, 0, v.nC);
        casePatchTable(c);
    } catch (...) { caseAbandon(c, 0); throw; }
    caseCount(c);
    *out = c;
    return QGD_OK;
    QGD_CATCH
}
int qgd_scalar_case_free(qgd_scalar_case_t c) {
    if (!c) return QGD_OK;
    (void)hipSetDevice(c->dev->deviceId);
    (void)hipStreamSynchronize(c->stream());   // (with or without a solver: no kernel of the last step still reads the arena)
    return caseAbandon(c, QGD_OK);
}
int qgd_scalar_case_set_bc(qgd_scalar_case_t c, int32_t patch, int32_t bcU, const double* valueU, int32_t bcT, double valueT) {
    QGD_TRY
    return casePatchEntry(c, "qgd_scalar_case_set_bc", patch, bcU, valueU, bcT, valueT, 0, QGD_BC_ZEROGRADIENT, 0.0);
    QGD_CATCH
}
int qgd_scalar_case_set_fields(qgd_scalar_case_t c, const double* U, const double* T) {
    QGD_TRY
    if (!c || !U || !T) return fail(QGD_ERR_INVALID, "qgd_scalar_case_set_fields: null argument");
    qgd_device_s* d = c->dev;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& m = d->view;
    if (!c->bc.empty()) HIP_CHECK(hipMemcpy(c->bcDev, c->bc.data(), sizeof(PatchBCDev) * c->bc.size(), hipMemcpyHostToDevice));
    Workspace& ws = d->ws;
    double* dU = ws.get<double>(WS_CELL, 3 * (size_t)m.nC);
    double* dT = ws.get<double>(WS_A, (size_t)m.nC);
    ws.h2d(dU, U, sizeof(double) * 3 * (size_t)m.nC, d->stream);
    ws.h2d(dT, T, sizeof(double) * (size_t)m.nC, d->stream);
    (void)hipGetLastError();
    launchScalarSetup(d->stream, m, c->view, c->bcDev, dU, dT, c->work, c->red);
    HIP_CHECK(hipGetLastError());
    double red[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(red, c->red, sizeof(red), hipMemcpyDeviceToHost, d->stream));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    c->maxUh = std::max(red[0], 0.0); c->minTau = red[1];
    c->dt = c->opt.deltaT; c->dtDiag = 0; c->CoNum = c->dt * c->maxUh; c->time = 0; c->steps = 0;
    if (c->implSolver) implicitStatsReset(c->implSolver);
    c->fieldsSet = true;
    return QGD_OK;
    QGD_CATCH
}
int qgd_scalar_case_step(qgd_scalar_case_t c, int32_t nSteps) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_scalar_case_step: call qgd_scalar_case_set_fields first");
    qgd_device_s* d = c->dev;
    HIP_CHECK(hipSetDevice(d->deviceId));
    const MeshView& m = d->view;
    const qgd_scalar_options& o = c->opt;
    for (int i = 0; i < nSteps; ++i) {
        c->CoNum = c->dt * c->maxUh;                                         // .C L88-92 (fixed deltaT: what the application prints)
        if (o.adjustTimeStep) {                                             // setDeltaT-QGDQHD.H L41-61
            const double maxDeltaTFact = o.maxCo / (c->CoNum + 1e-15);
            const double deltaTFact = std::min(std::min(maxDeltaTFact, 1.0 + 0.1 * maxDeltaTFact), 1.2);
            c->dt = std::min(deltaTFact * c->dt, std::min(o.maxDeltaT, o.cTau * c->minTau));
        }
        c->time += c->dt;                                                   // runTime++
        c->steps++;
        if (!o.implicitDiffusion) continue;                                 // .C L113: there is no else -- T stays as it is
        (void)hipGetLastError();
        if (c->dt != c->dtDiag) { launchScalarDiag(d->stream, m, c->view, c->dt); c->dtDiag = c->dt; }
        implicitStepMark(c->implSolver, true);
        launchScalarAssemble(d->stream, c->stencil, c->usesPoints, m, c->view, c->bcDev, c->dt, true);
        HIP_CHECK(hipGetLastError());
        implicitSolveSetup(c->implSolver, 1, 1, c->view.a, c->view.diag, c->view.rhs, c->view.T, o.implicitTol, o.implicitMaxIter);
        implicitSolveRun(c->implSolver, nullptr);
        implicitSolveEnd(c->implSolver, 1);
        implicitStepMark(c->implSolver, false);
        launchScalarPatchValues(d->stream, m, c->view, c->bcDev);            // solve() ends in correctBoundaryConditions()
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}
int qgd_scalar_case_get_field(qgd_scalar_case_t c, const char* name, double* out, int64_t outDoubles) {
    QGD_TRY
    if (!c || !name || !out) return fail(QGD_ERR_INVALID, "qgd_scalar_case_get_field: null argument");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_scalar_case_get_field: call qgd_scalar_case_set_fields first");
    qgd_device_s* d = c->dev;
    HIP_CHECK(hipSetDevice(d->deviceId));
    HIP_CHECK(hipStreamSynchronize(d->stream));
    const MeshView& m = d->view;
    const ScalarView& q = c->view;
    const std::string s(name);
    const size_t nF = (size_t)m.nF;
    const double* src = nullptr;
    int64_t count = 0;
    int nc = 1;          // > 1: src is SoA with stride nF, the caller gets nc per face
    if (s == "T") { src = q.T; count = m.nC; }
    else if (s == "T.boundary") { src = q.Tb; count = m.nBF; }
    else if (s == "phiu") { src = q.phiu; count = m.nF; }
    else if (s == "tauQGDf") { src = q.tauF; count = m.nF; }
    else if (s == "hQGDf") { src = m.hf; count = m.nF; }
    else if (s == "Uf") { src = q.Uf; count = m.nF; nc = 3; }
    else if (s == "gradTf" || s == "phiTf" || s == "phiTauTReg") {
        ScalarView qd = q;
        qd.dbg = d->ws.get<double>(WS_B, 5 * std::max<size_t>(nF, 1));
        (void)hipGetLastError();
        launchScalarAssemble(d->stream, c->stencil, c->usesPoints, m, qd, c->bcDev, c->dt, false);
        HIP_CHECK(hipGetLastError());
        count = m.nF;
        if (s == "gradTf") { src = qd.dbg; nc = 3; } else src = qd.dbg + (s == "phiTf" ? 3 : 4) * nF;
    } else return fail(QGD_ERR_INVALID, "qgd_scalar_case_get_field: unknown field " + s);
    if (count * nc > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
    if (count == 0) return QGD_OK;
    fetchFaceSoA(d, d->stream, src, count, nc, out);
    return QGD_OK;
    QGD_CATCH
}
int qgd_scalar_case_info(qgd_scalar_case_t c, double info[12]) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    for (int k = 0; k < 12; ++k) info[k] = 0.0;
    info[0] = c->time; info[1] = c->dt > 0 ? c->dt : c->opt.deltaT; info[2] = c->CoNum; info[3] = (double)c->steps;
    info[10] = c->maxUh; info[11] = c->minTau;
    if (c->implSolver && c->fieldsSet) {
        HIP_CHECK(hipSetDevice(c->dev->deviceId));
        int it[4] = {0, 0, 0, 0};
        double r0[4] = {0, 0, 0, 0}, r1[4] = {0, 0, 0, 0}, un = 0, stalled = 0;
        implicitSolverInfo(c->implSolver, it, r0, r1, &un, &stalled);   // the case's solve is kept in the second block (implicitSolveEnd(S, 1))
        info[4] = it[3]; info[5] = r0[3]; info[6] = r1[3]; info[7] = un; info[8] = stalled;
        info[9] = implicitSolverChebyshev(c->implSolver) ? 2.0 : 1.0;
    }
    return QGD_OK;
    QGD_CATCH
}
int qgd_scalar_case_sync(qgd_scalar_case_t c) { return caseSync(c); }

int qgd_comm_unique_id(void* id128) {
    QGD_TRY
    if (!id128) return fail(QGD_ERR_INVALID, "qgd_comm_unique_id: null argument");
    if (!rcclRef().why.empty()) return fail(QGD_ERR_NOT_IMPLEMENTED, rcclRef().why);
    ncclUniqueId id;
    RCCL_CHECK(rcclRef().getUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(id128, &id, sizeof(id));
    return QGD_OK;
    QGD_CATCH
}
int qgd_comm_create(int deviceId, int rank, int nRanks, const void* id128, qgd_comm_t* out) {
    QGD_TRY
    if (!out || !id128 || nRanks < 1 || rank < 0 || rank >= nRanks) return fail(QGD_ERR_INVALID, "qgd_comm_create: bad argument");
    if (!rcclRef().why.empty()) return fail(QGD_ERR_NOT_IMPLEMENTED, rcclRef().why);
    HIP_CHECK(hipSetDevice(deviceId));
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    qgd_comm_s* c = new qgd_comm_s();
    c->rank = rank; c->nRanks = nRanks; c->deviceId = deviceId;
    try { RCCL_CHECK(rcclRef().commInitRank(&c->comm, nRanks, id, rank)); }
    catch (...) { delete c; throw; }
    *out = c;
    return QGD_OK;
    QGD_CATCH
}
int qgd_comm_free(qgd_comm_t c) {
    if (!c) return QGD_OK;
    ncclResult_t r = ncclSuccess;
    if (c->comm && rcclRef().commDestroy) r = rcclRef().commDestroy(c->comm);
    delete c;
    if (r != ncclSuccess)
        return fail(QGD_ERR_HIP, std::string("qgd_comm_free: ncclCommDestroy: ") + (rcclRef().errorString ? rcclRef().errorString(r) : "RCCL error"));
    return QGD_OK;
}

int qgd_comm_info(qgd_comm_t c, int32_t info[3]) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, "qgd_comm_info: null argument");
    int rank = -1, count = -1, device = -1;
    RCCL_CHECK(rcclRef().commUserRank(c->comm, &rank));
    RCCL_CHECK(rcclRef().commCount(c->comm, &count));
    RCCL_CHECK(rcclRef().commCuDevice(c->comm, &device));
    info[0] = rank; info[1] = count; info[2] = device;
    return QGD_OK;
    QGD_CATCH
}

// the all-reduces of a solve across the ranks (SolveHooks::allreduce, ::allreduceBuf) over RCCL on `st`; none on one rank
static void rcclAllReduceHooks(SolveHooks& hooks, qgd_comm_s* comm, hipStream_t st) {
    if (!comm || comm->nRanks <= 1) return;
    hooks.allreduce = [comm, st](double* ptr, int n) { RCCL_CHECK(rcclRef().allReduce(ptr, ptr, (size_t)n, ncclFloat64, ncclSum, comm->comm, st)); };
    // the Chebyshev solves' spectral bound: MAX over the ranks (op 3; 2 = SUM)
    hooks.allreduceBuf = [comm, st](double* ptr, int64_t n, int op) {
        RCCL_CHECK(rcclRef().allReduce(ptr, ptr, (size_t)n, ncclFloat64, op == 3 ? ncclMax : ncclSum, comm->comm, st));
    };
}
int qgd_case_halo_exchange(qgd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (c->dev->halo.empty() || nSlots <= 0) return QGD_OK;  // unsharded: nothing to exchange
    if (!comm || !peers) return fail(QGD_ERR_INVALID, "qgd_case_halo_exchange: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    exchangeOn(c, comm, peers, nSlots, c->stream(), 0);
    return QGD_OK;  // stream-ordered on the case's stream
    QGD_CATCH
}
int qgd_case_allreduce_max(qgd_case_t c, qgd_comm_t comm) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!comm || comm->nRanks == 1) return QGD_OK;
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    RCCL_CHECK(rcclRef().allReduce(c->view.red, c->view.red, 2, ncclFloat64, ncclMax, comm->comm, c->stream()));
    return QGD_OK;
    QGD_CATCH
}
int qgd_case_step_sharded(qgd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int overlapped) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_step_sharded: call qgd_case_set_fields first");
    // (a case with species: on an unsharded device, which this entry steps like qgd_case_step, or with QGD_SPECIES_HALO on a shard, where the
    // state message carries the composition and stepAdvance's parts the species block -- nothing else differs)
    if (c->sp.nS) { const int rs = speciesReady(c, "qgd_case_step_sharded"); if (rs) return rs; }
    const bool sharded = !c->dev->halo.empty() && nSlots > 0;
    if (sharded && (!comm || !peers)) return fail(QGD_ERR_INVALID, "qgd_case_step_sharded: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const bool adjust = c->opt.adjustTimeStep != 0;
    if (sharded) checkHaloPeers(comm, peers, std::min<int>(nSlots, (int)c->dev->halo.size()));   // before the first message of the step
    if (sharded && midExchangeNeeded(c)) {
        stepAssemble(c, 1);
        exchangeOn(c, comm, peers, nSlots, c->stream(), 5);
        stepAssemble(c, 2);
    } else stepAssemble(c);
    if (adjust && comm && comm->nRanks > 1)
        RCCL_CHECK(rcclRef().allReduce(c->view.red, c->view.red, 2, ncclFloat64, ncclMax, comm->comm, c->stream()));
    if (!sharded) { stepAdvance(c, 0); HIP_CHECK(hipGetLastError()); return QGD_OK; }
    if (c->opt.implicitDiffusion) {
        // the reference's default branch on shards: the dot products of its four solves are ncclAllReduce of the control block, the
        // gradients, the new velocity and the search directions travel as grouped send/recv pairs, then the state message as usual
        SolveHooks hooks;
        hipStream_t st = c->stream();
        rcclAllReduceHooks(hooks, comm, st);
        auto halo = [&](int kind) { exchangeOn(c, comm, peers, nSlots, st, kind); };
        hooks.haloDirection = [&]() { halo(3); };
        hooks.haloGuess = [&]() { halo(4); };
        implicitAdvanceWith(c, &hooks, halo);
        halo(0);
        HIP_CHECK(hipGetLastError());
        return QGD_OK;
    }
    if (!overlapped) {
        stepAdvance(c, 0);
        exchangeOn(c, comm, peers, nSlots, c->stream(), 0);
    } else {
        // boundary layer first; pack / send / recv / unpack on the library's halo stream while the compute stream
        // updates the remaining cells; the next assembly waits for the unpack
        if (!c->ownHaloStream) {
            HIP_CHECK(hipStreamCreateWithFlags(&c->ownHaloStream, hipStreamNonBlocking));
            HIP_CHECK(hipEventCreateWithFlags(&c->evLayerDone, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&c->evUnpacked, hipEventDisableTiming));
        }
        stepAdvance(c, 1);
        HIP_CHECK(hipEventRecord(c->evLayerDone, c->stream()));
        HIP_CHECK(hipStreamWaitEvent(c->ownHaloStream, c->evLayerDone, 0));
        exchangeOn(c, comm, peers, nSlots, c->ownHaloStream, 0);
        HIP_CHECK(hipEventRecord(c->evUnpacked, c->ownHaloStream));
        stepAdvance(c, 2);
        HIP_CHECK(hipStreamWaitEvent(c->stream(), c->evUnpacked, 0));
    }
    HIP_CHECK(hipGetLastError());
    return QGD_OK;  // stream-ordered: qgd_case_stream_sync waits
    QGD_CATCH
}

// ---- the QHD case over the library's own transport ----------------------------------------------------------------------
// every message kind on the device's stream
static void exchangeOn(qgd_qhd_case_s* c, qgd_comm_s* comm, const int32_t* peers, int nSlots, int kind) {
    exchangeOn(c->dev, comm, peers, nSlots, c->dev->stream, haloMessage(c, kind), haloBuffers(c));
}
int qgd_qhd_case_halo_exchange(qgd_qhd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int kind) {
    QGD_TRY
    if (!c || kind < 0 || kind > 4) return fail(QGD_ERR_INVALID, "bad argument");
    if (c->dev->halo.empty() || nSlots <= 0) return QGD_OK;
    if (!comm || !peers) return fail(QGD_ERR_INVALID, "qgd_qhd_case_halo_exchange: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    exchangeOn(c, comm, peers, nSlots, kind);
    return QGD_OK;
    QGD_CATCH
}
// one QHDFoam step of a sharded case [QHDFoam_8C L83-139]: the dot products of the pressure solve are ncclAllReduce of the
// control block, its search direction and the states travel as grouped send/recv pairs; the only host waits are the
// run-ahead checks of the solve (pressureSolveRun)
int qgd_qhd_case_step_sharded(qgd_qhd_case_t c, qgd_comm_t comm, const int32_t* peers, int nSlots, int32_t nSteps) {
    QGD_TRY
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_qhd_case_step_sharded: call qgd_qhd_case_set_fields first");
    if (c->adjust) return fail(QGD_ERR_NOT_IMPLEMENTED, "qgd_qhd_case_step_sharded: adjustTimeStep (qgd_qhd_case_set_time_control) is served by qgd_qhd_case_step alone");
    qgd_device_s* d = c->dev;
    const bool sharded = !d->halo.empty() && nSlots > 0;
    if (sharded && (!comm || !peers)) return fail(QGD_ERR_INVALID, "qgd_qhd_case_step_sharded: null argument");
    HIP_CHECK(hipSetDevice(d->deviceId));
    if (sharded) checkHaloPeers(comm, peers, std::min<int>(nSlots, (int)d->halo.size()));
    SolveHooks hooks;
    rcclAllReduceHooks(hooks, comm, d->stream);
    if (sharded) hooks.haloDirection = [&]() { exchangeOn(c, comm, peers, nSlots, 2); };
    if (sharded) hooks.haloMg = [&]() { exchangeOn(c, comm, peers, nSlots, 3); };
    std::function<void(int)> haloState;
    if (sharded) haloState = [&](int kind) { exchangeOn(c, comm, peers, nSlots, kind); };
    for (int i = 0; i < nSteps; ++i) qhdStepWith(c, &hooks, haloState);
    HIP_CHECK(hipStreamSynchronize(d->stream));
    return QGD_OK;
    QGD_CATCH
}

// ---- accessors --------------------------------------------------------------------
int qgd_case_get_field(qgd_case_t c, const char* name, double* out, int64_t outDoubles) {
    QGD_TRY
    if (!c || !name || !out) return fail(QGD_ERR_INVALID, "qgd_case_get_field: null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    const MeshView& m = c->dev->view;
    const GasModel& g = c->gas;
    std::string s(name);
    const bool bnd = boundaryName(s);
    // face fields from the debug buffer
    static const std::map<std::string, std::pair<int, int>> faceSlots = {
        {"phiJm", {DBG_PHIJM, 1}}, {"phiJmU", {DBG_PHIJMU, 3}}, {"phiP", {DBG_PHIP, 3}}, {"phiPi", {DBG_PHIPI, 3}},
        {"phiJmH", {DBG_PHIJMH, 1}}, {"phiQ", {DBG_PHIQ, 1}}, {"phiPiU", {DBG_PHIPIU, 1}}, {"phiwStar", {DBG_PHIW, 1}},
        {"phi", {DBG_PHI, 1}}, {"tauQGDf", {DBG_TAU, 1}}, {"gradUf", {DBG_GRADU, 9}}, {"gradef", {DBG_GRADE, 3}},
        {"gradRhof", {DBG_GRADRHO, 3}}, {"gradPf", {DBG_GRADP, 3}}};
    if (!bnd && s == "hQGDf") {
        if ((int64_t)c->dev->hf.size() > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        std::copy(c->dev->hf.begin(), c->dev->hf.end(), out);
        return QGD_OK;
    }
    // face fields of the implicitDiffusion branch, as the last step left them [updateFluxes.H L107-111, QGDUEqn.H L72-74]
    if (!bnd && (s == "phiTauMC" || s == "phiSigmaDotU")) {
        if (!c->impl.phiTau) return fail(QGD_ERR_INVALID, "qgd_case_get_field: " + s + " exists with implicitDiffusion true only");
        const int nc = s == "phiTauMC" ? 3 : 1;
        if ((int64_t)m.nF * nc > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        HIP_CHECK(hipStreamSynchronize(c->stream()));
        // stored at the faces' slot-major positions (qgd_implicit.hip implFaceKernel): internal face f at fpos[f], patch faces at their label
        std::vector<double> tmp((size_t)m.nF);
        std::vector<int32_t> fpos((size_t)m.nIF);
        if (m.nIF) HIP_CHECK(hipMemcpy(fpos.data(), m.fpos, sizeof(int32_t) * (size_t)m.nIF, hipMemcpyDeviceToHost));
        for (int k = 0; k < nc; ++k) {
            const double* src = nc == 3 ? c->impl.phiTau + (size_t)k * m.nF : c->impl.phiSig;
            HIP_CHECK(hipMemcpy(tmp.data(), src, sizeof(double) * (size_t)m.nF, hipMemcpyDeviceToHost));
            for (int64_t f = 0; f < m.nF; ++f) out[f * nc + k] = tmp[f < m.nIF ? (size_t)fpos[f] : (size_t)f];
        }
        return QGD_OK;
    }
    auto fs = faceSlots.find(s);
    if (!bnd && fs != faceSlots.end()) {
        if (!c->dbgBuf) return fail(QGD_ERR_INVALID, "face fields are materialised by qgd_case_update_fluxes; call it first");
        const int slot = fs->second.first, nc = fs->second.second;
        if ((int64_t)m.nF * nc > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        fetchFaceSoA(c->dev, c->stream(), c->dbgBuf + (size_t)slot * m.nF, m.nF, nc, out);
        return QGD_OK;
    }
    // cell / boundary fields: extracted from the records on the device, one dense copy back
    static const std::map<std::string, int> cellFields = {
        {"rho", XF_RHO}, {"U", XF_U}, {"p", XF_P}, {"e", XF_E}, {"T", XF_T}, {"rhoU", XF_RHOU}, {"rhoE", XF_RHOE}, {"c", XF_C},
        {"psi", XF_PSI}, {"mu", XF_MU}, {"alphau", XF_ALPHAU}, {"tauQGD", XF_TAUQGD}, {"muQGD", XF_MUQGD},
        {"alphauQGD", XF_ALPHAUQGD}, {"hQGD", XF_HQGD}, {"H", XF_H}, {"gamma", XF_GAMMA}};
    if (s == "ScQGD") {   // the uniform value repeated, the array of qgd_case_set_qgd_coeffs, or the sensor's last result
        const int64_t n = bnd ? m.nBF : m.nC;
        if (n > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
        const double* src = bnd ? c->view.scb : c->view.sc;
        if (src && n) HIP_CHECK(hipMemcpy(out, src, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
        else std::fill(out, out + n, g.ScQGD);
        return QGD_OK;
    }
    auto cf = cellFields.find(s);
    if (cf == cellFields.end()) return fail(QGD_ERR_UNKNOWN_NAME, "qgd_case_get_field: unknown field " + s);
    const int64_t n = bnd ? m.nBF : m.nC;
    const int nc = (cf->second == XF_U || cf->second == XF_RHOU) ? 3 : 1;
    if (n * nc > outDoubles) return fail(QGD_ERR_INVALID, "output too small");
    if (n == 0) return QGD_OK;
    double* tmp = nullptr;
    HIP_CHECK(hipMalloc((void**)&tmp, sizeof(double) * (size_t)(n * nc)));
    try {
        (void)hipGetLastError();
        launchExtractField(c->stream(), bnd ? c->view.bA : c->view.A, bnd ? c->view.bB : c->view.B, bnd ? nullptr : c->view.rE,
                           bnd ? m.hQGDb : m.hQGD, bnd ? c->view.aQb : c->view.aQ, n, g, cf->second, tmp);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(c->stream()));
        HIP_CHECK(hipMemcpy(out, tmp, sizeof(double) * (size_t)(n * nc), hipMemcpyDeviceToHost));
    } catch (...) { (void)hipFree(tmp); throw; }
    (void)hipFree(tmp);
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_info(qgd_case_t c, double info[6]) {
    QGD_TRY
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    Launcher L = launcherOf(c);
    L.pre = nullptr; L.post = nullptr;
    (void)hipGetLastError();
    launchCellMinReduce(L, c->view);  // min(rho), min(e) since the previous query [QGDFoam_8C L142]
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    double red[4], dt[3];
    HIP_CHECK(hipMemcpy(red, c->view.red, sizeof(red), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(dt, c->view.dt, sizeof(dt), hipMemcpyDeviceToHost));
    info[0] = c->opt.adjustTimeStep ? dt[1] : c->time;
    info[1] = dt[0];
    info[2] = dt[2];
    info[3] = red[2];
    info[4] = red[3];
    info[5] = (double)c->steps;
    return QGD_OK;
    QGD_CATCH
}

int qgd_case_fused_info(qgd_case_t c, int64_t info[8]) {
    if (!c || !info) return fail(QGD_ERR_INVALID, "null argument");
    const MeshView& v = c->dev->view;
    const bool fusedImpl = implFusedNow(c);   // (off while the case carries per-face velocities on a fixedValue patch)
    info[0] = c->fused ? 1 : (fusedImpl ? 2 : (c->fusedAdj ? 3 : 0));   // 2: the implicitDiffusion branch's block-fused assembly of the U systems; 3: Courant-number control (blocks up to their sums + a cell kernel)
    info[1] = (c->fused || fusedImpl || c->fusedAdj) ? v.fuBlocks : 0;
    info[2] = c->fused ? c->dev->fusedFacesComputed : 0;
    info[3] = (c->fused || c->fusedAdj) ? v.fuLds : (fusedImpl ? v.fuLdsImpl : 0);
    info[4] = c->fused ? c->dev->fusedCellsStaged : 0;
    info[5] = c->fused ? c->dev->fusedCellsStagedFull : 0;
    info[6] = c->fused ? c->dev->fusedVertsStaged : 0;
    info[7] = c->fused ? v.fuLayerBlocks : 0;
    return QGD_OK;
}

int qgd_case_implicit_info(qgd_case_t c, double info[16]) { return caseImplicitInfo(c, "null argument", true, info); }
int qgd_case_implicit_apply_time(qgd_case_t c, int reps, double info[2]) {
    QGD_TRY
    if (!c || !info || reps <= 0) return fail(QGD_ERR_INVALID, "bad argument");
    if (!c->implSolver || !c->fieldsSet) return fail(QGD_ERR_INVALID, "qgd_case_implicit_apply_time: an implicitDiffusion case after qgd_case_set_fields");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    implicitSolverSetStream(c->implSolver, c->stream());
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    (void)hipGetLastError();
    int rows = 0;
    info[0] = implicitApplyMs(c->implSolver, c->impl, reps, &rows);
    info[1] = rows;
    return QGD_OK;
    QGD_CATCH
}
// the control block of the solve in flight: a sharded run SUM-reduces control[0..12), [12..16), [16..20), [20..24), [24..32) after solver
// phases 0, 1, 2, 3, 4
int qgd_case_implicit_control(qgd_case_t c, double control[68], int set) { return caseImplicitControl(c, "bad argument", control, set); }
int qgd_case_implicit_control_ptr(qgd_case_t c, void** devicePtr) { return caseImplicitControlPtr(c, "bad argument", devicePtr); }
int qgd_case_implicit_solve_status(qgd_case_t c, double status[2]) { return caseImplicitSolveStatus(c, "bad argument", 3, status); }

int qgd_struct_sizes(int64_t sizes[4]) {
    if (!sizes) return fail(QGD_ERR_INVALID, "null argument");
    sizes[0] = (int64_t)sizeof(qgd_case_options); sizes[1] = (int64_t)sizeof(qgd_qhd_options);
    sizes[2] = (int64_t)sizeof(qgd_poisson_control); sizes[3] = QGD_ABI_VERSION;
    return QGD_OK;
}

// ---- measurement -------------------------------------------------------------------
int qgd_case_timing(qgd_case_t c, int enable) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    if (!enable) harvestTiming(c);
    c->timing = enable != 0;
    return QGD_OK;
}
int qgd_case_kernel_time(qgd_case_t c, int k, double* totalMs, int64_t* launches) {
    if (!c || k < 0 || k >= QGD_K_COUNT || !totalMs || !launches) return fail(QGD_ERR_INVALID, "bad argument");
    (void)hipSetDevice(c->dev->deviceId);
    harvestTiming(c);
    *totalMs = c->totalMs[k];
    *launches = c->launches[k];
    return QGD_OK;
}
int qgd_case_timing_reset(qgd_case_t c) {
    if (!c) return fail(QGD_ERR_INVALID, "null case");
    (void)hipSetDevice(c->dev->deviceId);
    harvestTiming(c);
    for (int k = 0; k < QGD_K_COUNT; ++k) { c->totalMs[k] = 0; c->launches[k] = 0; }
    return QGD_OK;
}
int qgd_case_device_bytes(qgd_case_t c, int64_t* bytes) {
    if (!c || !bytes) return fail(QGD_ERR_INVALID, "null argument");
    *bytes = c->arena.bytes + c->dev->arena.bytes;
    return QGD_OK;
}

// ---------------------------------------------------------------------------
// run monitors (qgd_monitor.hip)
// ---------------------------------------------------------------------------
static const char* patchTypeWord(int t) {
    switch (t) {
        case QGD_PATCH_EMPTY: return "empty";
        case QGD_PATCH_WEDGE: return "wedge";
        case QGD_PATCH_CYCLIC: return "cyclic";
        case QGD_PATCH_HALO: return "halo";
        default: return "real";
    }
}

// the checks of a specification and the handle both kinds of monitor share; `who` names the entry in the messages.  Returns an error code
// (out untouched) or QGD_OK with the handle filled in but for its case.
static int monitorBuild(const std::string& who, qgd_device_s* d, const qgd_monitor_spec* spec, const MonitorShape& shape, qgd_monitor_s** out) {
    if (spec->nProbes < 0 || spec->nPatches < 0 || (spec->nProbes > 0 && !spec->probeCells) || (spec->nPatches > 0 && !spec->patches))
        return fail(QGD_ERR_INVALID, who + ": bad specification (negative count or null list)");
    const MeshView& m = d->view;
    for (int32_t i = 0; i < spec->nProbes; ++i)
        if (spec->probeCells[i] < -1 || spec->probeCells[i] >= m.nC)
            return fail(QGD_ERR_INVALID, who + ": probe " + std::to_string(i) + ": cell label " + std::to_string(spec->probeCells[i]) +
                                             " is out of range [0, " + std::to_string(m.nC) + ") (-1 = not on this rank)");
    for (int32_t i = 0; i < spec->nPatches; ++i) {
        const int32_t p = spec->patches[i];
        if (p < 0 || p >= (int32_t)d->patches.size())
            return fail(QGD_ERR_INVALID, who + ": patch index " + std::to_string(p) + " is out of range [0, " + std::to_string(d->patches.size()) + ")");
        const int t = d->patches[p].type;
        if (t == QGD_PATCH_HALO || t == QGD_PATCH_EMPTY || t == QGD_PATCH_CYCLIC || t == QGD_PATCH_WEDGE)
            return fail(QGD_ERR_INVALID, who + ": patch " + std::to_string(p) + " ('" + d->patches[p].name + "') is a " + patchTypeWord(t) +
                                             " patch: it carries no boundary fluxes of its own (patch totals are formed on real patches only)");
    }
    HIP_CHECK(hipSetDevice(d->deviceId));
    // the faces of the requested patches that carry fields and belong to an owned cell, patch by patch in label order, cut into chunks
    // of at most 256 that never span two patches
    std::vector<uint8_t> fkind((size_t)m.nBF);
    std::vector<int32_t> own((size_t)m.nBF);
    if (m.nBF) {
        HIP_CHECK(hipMemcpy(fkind.data(), m.fkind + m.nIF, (size_t)m.nBF, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(own.data(), m.own + m.nIF, sizeof(int32_t) * (size_t)m.nBF, hipMemcpyDeviceToHost));
    }
    std::vector<int32_t> faceList, chunkStart{0}, patchChunk{0};
    for (int32_t i = 0; i < spec->nPatches; ++i) {
        const Patch& pt = d->patches[spec->patches[i]];
        int32_t inChunk = 0;
        for (int32_t f = pt.start; f < pt.start + pt.size; ++f) {
            const int32_t b = f - m.nIF;
            if (b < 0 || b >= m.nBF) throw std::invalid_argument(who + ": patch '" + pt.name + "' has faces outside the boundary range");
            if (fkind[b] == FK_SKIP || own[b] < d->ownedBegin || own[b] >= d->ownedEnd) continue;
            if (inChunk == 256) { chunkStart.push_back((int32_t)faceList.size()); inChunk = 0; }
            faceList.push_back(b);
            ++inChunk;
        }
        if (inChunk > 0) chunkStart.push_back((int32_t)faceList.size());
        patchChunk.push_back((int32_t)chunkStart.size() - 1);
    }
    qgd_monitor_s* mo = new qgd_monitor_s();
    try {
        MonitorView& v = mo->view;
        DeviceArena& a = mo->arena;
        v.ownedBegin = d->ownedBegin; v.ownedEnd = d->ownedEnd;
        v.cellGlobal = a.upload(d->cellGlobal); v.cellGlobalOffset = d->cellGlobalOffset;
        v.cellPart = a.alloc<double>((size_t)QGD_MONITOR_BLOCKS * shape.cellRow());
        v.nProbes = spec->nProbes;
        v.probeCell = a.upload(std::vector<int32_t>(spec->probeCells, spec->probeCells + spec->nProbes));
        v.nPatches = spec->nPatches; v.nChunks = (int32_t)chunkStart.size() - 1;
        v.faceList = a.upload(faceList); v.chunkStart = a.upload(chunkStart); v.patchChunk = a.upload(patchChunk);
        v.patchPart = a.alloc<double>((size_t)std::max(1, v.nChunks) * shape.patchRow);
        v.off[0] = 0; v.off[1] = 8; v.off[2] = v.off[1] + shape.sums; v.off[3] = v.off[2] + 4 * shape.extrema;
        v.off[4] = v.off[3] + (int64_t)shape.probeRow * v.nProbes;
        mo->nDoubles = v.off[4] + (int64_t)shape.patchRow * v.nPatches;
        mo->result = a.alloc<double>((size_t)mo->nDoubles);
        HIP_CHECK(hipHostMalloc((void**)&mo->host, sizeof(double) * (size_t)mo->nDoubles * QGD_MONITOR_SLOTS, hipHostMallocDefault));
        for (int k = 0; k < QGD_MONITOR_SLOTS; ++k) HIP_CHECK(hipEventCreateWithFlags(&mo->ev[k], hipEventDisableTiming));
    } catch (...) {
        for (hipEvent_t e : mo->ev) if (e) (void)hipEventDestroy(e);
        if (mo->host) (void)hipHostFree(mo->host);
        mo->arena.release();
        delete mo;
        throw;
    }
    *out = mo;
    return QGD_OK;
}
// what the two create entries share: `who` names the entry, `setFields` the call it asks for first, `qhd` the kind of the case
static int monitorCreate(const char* who, const char* setFields, CaseCore* c, bool qhd, const qgd_monitor_spec* spec, const MonitorShape& shape,
                         qgd_monitor_s** out) {
    QGD_TRY
    if (!c || !spec || !out) return fail(QGD_ERR_INVALID, std::string(who) + ": null argument");
    if (!c->fieldsSet) return fail(QGD_ERR_INVALID, std::string(who) + ": call " + setFields + " first (a monitor samples the state the case holds)");
    qgd_monitor_s* mo = nullptr;
    const int rc = monitorBuild(who, c->dev, spec, shape, &mo);
    if (rc) return rc;
    mo->c = c; mo->qhd = qhd;
    g_monitors.push_back(mo);
    c->monitors.push_back(mo);
    *out = mo;
    return QGD_OK;
    QGD_CATCH
}
int qgd_monitor_create(qgd_case_t c, const qgd_monitor_spec* spec, qgd_monitor_t* out) {
    return monitorCreate("qgd_monitor_create", "qgd_case_set_fields", c, false, spec, kFlowMonitorShape, out);
}
// the monitor of a QHD case (qgd_qhd_monitor.hip): the same handle, served by the entries below
int qgd_qhd_monitor_create(qgd_qhd_case_t c, const qgd_monitor_spec* spec, qgd_monitor_t* out) {
    return monitorCreate("qgd_qhd_monitor_create", "qgd_qhd_case_set_fields", c, true, spec, kQhdMonitorShape, out);
}
int qgd_monitor_layout(qgd_monitor_t m, int64_t offsets[QGD_MONITOR_SECTIONS], int64_t* nDoubles, int32_t* gridCap) {
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_layout: not an open monitor (a monitor is freed with its case)");
    if (offsets) for (int k = 0; k < QGD_MONITOR_SECTIONS; ++k) offsets[k] = m->view.off[k];
    if (nDoubles) *nDoubles = m->nDoubles;
    if (gridCap) *gridCap = QGD_MONITOR_BLOCKS;
    return QGD_OK;
}
int qgd_monitor_sample(qgd_monitor_t m, int32_t slot) {
    QGD_TRY
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_sample: not an open monitor (a monitor is freed with its case)");
    if (slot < 0 || slot >= QGD_MONITOR_SLOTS) return fail(QGD_ERR_INVALID, "qgd_monitor_sample: slot must be 0.." + std::to_string(QGD_MONITOR_SLOTS - 1));
    CaseCore* core = m->c;
    if (!core->fieldsSet)
        return fail(QGD_ERR_INVALID, m->qhd ? "qgd_monitor_sample: the case's boundary conditions changed: call qgd_qhd_case_set_fields first"
                                            : "qgd_monitor_sample: the case's boundary conditions or coefficients changed: call qgd_case_set_fields first");
    HIP_CHECK(hipSetDevice(core->dev->deviceId));
    hipStream_t st = core->stream();
    (void)hipGetLastError();
    if (m->qhd) {   // a QHD case: three launches
        qgd_qhd_case_s* qc = static_cast<qgd_qhd_case_s*>(core);
        const int fluxState = qc->steps == 0 ? 0 : (qc->view.implicit ? 2 : 1);
        launchQhdMonitorSample(st, m->view, qc->dev->view, qc->view, fluxState, m->result);   // (the view as it stands now: the fused advance swaps c4)
        HIP_CHECK(hipGetLastError());
    } else {
        qgd_case_s* c = static_cast<qgd_case_s*>(core);
        const int fluxState = !c->fluxAssembled ? 0 : (c->opt.implicitDiffusion ? 2 : 1);
        launchMonitorSample(st, m->view, c->dev->view, c->view, c->gas, fluxState, m->result);   // (the view as it stands now: the fused step swaps A / B)
        HIP_CHECK(hipGetLastError());
        if (m->spDoubles) {   // the species block: three more launches, behind the flow block in the same device buffer, so one copy takes both
            const int spState = !c->spFluxesValid ? 0 : (c->opt.implicitDiffusion ? 2 : 1);
            launchMonitorSpeciesSample(st, m->view, m->spView, c->dev->view, c->view, c->sp, c->spImpl.aF, spState, m->result + m->nDoubles);
            HIP_CHECK(hipGetLastError());
        }
    }
    // the copy into the slot follows on the same stream (a QHD monitor has no species block: spDoubles == 0)
    const size_t slotDoubles = (size_t)(m->nDoubles + m->spDoubles);
    HIP_CHECK(hipMemcpyAsync(m->host + (size_t)slot * slotDoubles, m->result, sizeof(double) * slotDoubles, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(m->ev[slot], st));
    m->sampled[slot] = true; m->time[slot] = core->time; m->step[slot] = core->steps;
    return QGD_OK;
    QGD_CATCH
}
int qgd_monitor_read(qgd_monitor_t m, int32_t slot, double* out, int64_t cap, double* time, int64_t* step) {
    QGD_TRY
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_read: not an open monitor (a monitor is freed with its case)");
    if (slot < 0 || slot >= QGD_MONITOR_SLOTS) return fail(QGD_ERR_INVALID, "qgd_monitor_read: slot must be 0.." + std::to_string(QGD_MONITOR_SLOTS - 1));
    if (!out || cap < m->nDoubles) return fail(QGD_ERR_INVALID, "qgd_monitor_read: output too small (qgd_monitor_layout gives the doubles of a result block)");
    if (!m->sampled[slot]) return fail(QGD_ERR_INVALID, "qgd_monitor_read: slot " + std::to_string(slot) + " was never sampled");
    HIP_CHECK(hipSetDevice(m->c->dev->deviceId));
    HIP_CHECK(hipEventSynchronize(m->ev[slot]));
    const double* src = m->host + (size_t)slot * (size_t)(m->nDoubles + m->spDoubles);
    std::copy(src, src + m->nDoubles, out);
    const bool adjusts = !m->qhd && static_cast<qgd_case_s*>(m->c)->opt.adjustTimeStep;
    if (time) *time = adjusts ? src[7] : m->time[slot];   // (a QHD case steps at a fixed deltaT; its header[7] holds flags)
    if (step) *step = m->step[slot];
    return QGD_OK;
    QGD_CATCH
}
// the species block of a monitor: sampled by the same qgd_monitor_sample, behind the flow block of the slot
int qgd_monitor_enable_species(qgd_monitor_t m) {
    QGD_TRY
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_enable_species: not an open monitor (a monitor is freed with its case)");
    if (m->qhd) return fail(QGD_ERR_INVALID, "qgd_monitor_enable_species: the monitor of a QHD case has no species block (QHDFoam and SRFQHDFoam carry no species)");
    qgd_case_s* c = static_cast<qgd_case_s*>(m->c);
    if (!c->sp.nS) return fail(QGD_ERR_INVALID, "qgd_monitor_enable_species: the case carries no species (qgd_case_set_species)");
    if (m->spDoubles) return QGD_OK;
    for (bool s : m->sampled)
        if (s) return fail(QGD_ERR_INVALID, "qgd_monitor_enable_species: call it before the monitor's first qgd_monitor_sample (the slots grow by the species block)");
    HIP_CHECK(hipSetDevice(c->dev->deviceId));
    const MonitorView& v = m->view;
    SpeciesMonitorView sm{};
    const int64_t nS = c->sp.nS, nOwned = (int64_t)v.ownedEnd - v.ownedBegin, tile = 256 * QGD_MONITOR_SPECIES_CELLS;
    sm.nRows = (int32_t)std::min<int64_t>((nOwned + tile - 1) / tile, QGD_MONITOR_BLOCKS);   // workgroups of the cell pass: they stride over the tiles beyond that
    sm.off[0] = 0; sm.off[1] = QGD_MONITOR_SPECIES_HEADER; sm.off[2] = sm.off[1] + nS; sm.off[3] = sm.off[2] + 4 * nS;
    sm.off[4] = sm.off[3] + nS * v.nProbes;
    const int64_t spDoubles = sm.off[4] + nS * v.nPatches;
    sm.cellPart = m->arena.alloc<double>((size_t)std::max(1, sm.nRows) * (size_t)(5 * nS + 3));
    sm.patchPart = m->arena.alloc<double>((size_t)std::max(1, v.nChunks) * (size_t)nS);
    double* result = m->arena.alloc<double>((size_t)(m->nDoubles + spDoubles));   // both blocks, the flow block first (its own buffer stays behind unused)
    double* host = nullptr;
    HIP_CHECK(hipHostMalloc((void**)&host, sizeof(double) * (size_t)(m->nDoubles + spDoubles) * QGD_MONITOR_SLOTS, hipHostMallocDefault));
    HIP_CHECK(hipStreamSynchronize(c->stream()));
    if (m->host) (void)hipHostFree(m->host);
    m->host = host;
    m->result = result;
    m->spView = sm;
    m->spDoubles = spDoubles;
    return QGD_OK;
    QGD_CATCH
}
int qgd_monitor_species_layout(qgd_monitor_t m, int64_t offsets[QGD_MONITOR_SECTIONS], int64_t* nDoubles) {
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_species_layout: not an open monitor (a monitor is freed with its case)");
    if (!m->spDoubles) return fail(QGD_ERR_INVALID, "qgd_monitor_species_layout: the species block is not enabled (qgd_monitor_enable_species)");
    if (offsets) for (int k = 0; k < QGD_MONITOR_SECTIONS; ++k) offsets[k] = m->spView.off[k];
    if (nDoubles) *nDoubles = m->spDoubles;
    return QGD_OK;
}
int qgd_monitor_species_read(qgd_monitor_t m, int32_t slot, double* out, int64_t cap) {
    QGD_TRY
    if (!monitorLive(m)) return fail(QGD_ERR_INVALID, "qgd_monitor_species_read: not an open monitor (a monitor is freed with its case)");
    if (!m->spDoubles) return fail(QGD_ERR_INVALID, "qgd_monitor_species_read: the species block is not enabled (qgd_monitor_enable_species)");
    if (slot < 0 || slot >= QGD_MONITOR_SLOTS) return fail(QGD_ERR_INVALID, "qgd_monitor_species_read: slot must be 0.." + std::to_string(QGD_MONITOR_SLOTS - 1));
    if (!out || cap < m->spDoubles)
        return fail(QGD_ERR_INVALID, "qgd_monitor_species_read: output too small (qgd_monitor_species_layout gives the doubles of a species block: " +
                                         std::to_string(m->spDoubles) + ")");
    if (!m->sampled[slot]) return fail(QGD_ERR_INVALID, "qgd_monitor_species_read: slot " + std::to_string(slot) + " was never sampled");
    HIP_CHECK(hipSetDevice(m->c->dev->deviceId));
    HIP_CHECK(hipEventSynchronize(m->ev[slot]));
    const double* src = m->host + (size_t)slot * (size_t)(m->nDoubles + m->spDoubles) + m->nDoubles;
    std::copy(src, src + m->spDoubles, out);
    return QGD_OK;
    QGD_CATCH
}
int qgd_monitor_free(qgd_monitor_t m) {
    if (!monitorLive(m)) return QGD_OK;   // null, or freed with its case
    (void)hipSetDevice(m->c->dev->deviceId);
    (void)hipStreamSynchronize(m->c->stream());
    std::vector<qgd_monitor_s*>& open = m->c->monitors;
    open.erase(std::remove(open.begin(), open.end(), m), open.end());
    monitorDestroy(m);
    return QGD_OK;
}

}  // extern "C"
