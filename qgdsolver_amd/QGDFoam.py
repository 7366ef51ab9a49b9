"""``python -m qgdsolver_amd.QGDFoam -case <dir>``: the explicit branch of the QGDFoam application
(QGDFoam.C L63-163) run from an OpenFOAM case directory on one MI355X.

What the reference's ``main`` does per step -- updateFields.H, updateFluxes.H, QGDCourantNo.H,
setDeltaT-QGDQHD.H, the three explicit equations, thermo.correct(), runTime.write() -- is
``QGDFoamCase.step`` plus ``foamfile.write_cell_fields`` (write_time's job from gathered fields) here, inside ``apprun.step_chunks``;
the run control, the stepping around the function objects and the report of the implicit solves are apprun's too.  Read from system/controlDict:
startFrom/startTime, endTime, deltaT, writeControl (timeStep, or runTime/adjustableRunTime with a
fixed deltaT), writeInterval, adjustTimeStep/maxCo/maxDeltaT, timePrecision, and of ``functions{}`` the types
probes, fieldMinMax, qgdIntegrals and qgdPatchFluxes, with species names among the fields and qgdSpeciesIntegrals and
qgdSpeciesPatchFluxes in a case with species (foamfile.read_functions; files under postProcessing/).
"""
import os
import sys
import time as _time

import numpy as np

from . import apprun
from . import foamfile as ff
from .apprun import find_start_time, time_name                     # (their names here: they lived in this module before apprun)
from .foamfile import write_cell_fields as _write_cell_fields      # (likewise)


def _distributed():
    """(rank, world, local_rank) from the torch.distributed.run environment"""
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def run(case_dir, n_steps=None, device_id=0, write=True, log=print, renumber="none", backend="nccl"):
    """One rank of the run.  With WORLD_SIZE > 1 (``python -m torch.distributed.run ... -m qgdsolver_amd.QGDFoam``) the
    undecomposed case is read by every rank, relabelled (``renumber``: none | rcm | morton), cut into contiguous cell
    ranges (``PolyMesh.shard``) and advanced with one halo message per neighbouring rank per step (``halo.RangeHalo``
    over RCCL; backend "gloo" stages the messages through host memory and lets all ranks share GPU 0: a debugging
    aid).  Rank 0 gathers the owned cells and writes the time directories in the case's own cell order."""
    rank, world, local_rank = _distributed()
    if rank != 0:
        log = lambda *a, **k: None  # noqa: E731
    cd = ff.read_dict(os.path.join(case_dir, "system", "controlDict"))
    t0, t0_name = find_start_time(case_dir, cd)
    from .fvsc import Device
    from .qgdfoam import QGDFoamCase, default_options

    gmesh, opt, fields, bcs = ff.read_case_setup(case_dir, t0_name)
    n_global = gmesh.nCells
    new_of_old = np.arange(n_global, dtype=np.int32)
    if renumber != "none":
        new_of_old = gmesh.rcm_order() if renumber == "rcm" else gmesh.morton_order()
        gmesh.renumber(new_of_old)
    old_of_new = np.argsort(new_of_old)
    dist = halo = torch = None
    if world > 1:
        import torch
        import torch.distributed as dist
        from .halo import HostStaged, RangeHalo

        staged = backend == "gloo"
        device_id = 0 if staged else local_rank
        torch.cuda.set_device(device_id)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if staged:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", device_id))
        mesh = gmesh.shard(world, rank)
        cells = old_of_new[mesh.array("cellGlobal")]  # labels in the case files of the shard's cells
        lo, hi = (n_global * rank) // world, (n_global * (rank + 1)) // world
        owned = (mesh.array("cellGlobal") >= lo) & (mesh.array("cellGlobal") < hi)
    else:
        mesh, cells, owned = gmesh, old_of_new, np.ones(n_global, dtype=bool)
    species = opt.get("species")
    species_halo = bool(species) and (world > 1 or bool(getattr(gmesh, "cyclic_pairs", None)))
    if species_halo and opt.get("implicitDiffusion"):
        # (named ahead of the flow's own refusal of cyclic patches with implicitDiffusion below)
        raise ff.FoamFileError(f"{case_dir}: species with implicitDiffusion true run on one rank, on a mesh without cyclic patches (the batched species "
                               f"solves are not distributed): this case has {world} rank(s)"
                               + (" and cyclic patches" if getattr(gmesh, "cyclic_pairs", None) else "") + "; use QGD { implicitDiffusion false; }")
    if getattr(gmesh, "cyclic_pairs", None):
        # translational cyclic pairs: the halves are glued, translated copies of the cells behind either half are refreshed by the library
        # after every step (PolyMesh.unroll_cyclic, DESIGN 6 "cyclic patches"); real cells keep their labels, the copies follow them
        if world > 1 or opt.get("implicitDiffusion") or renumber != "none":
            raise ff.FoamFileError(f"{case_dir}: a case with cyclic patches runs on one rank, explicit branch (QGD {{ implicitDiffusion false; }}), "
                                   "in the case's own cell order")
        if "alphaQGD" in fields or "ScQGD" in fields:   # (foamfile.load_case refuses the same case; before any device exists)
            raise ff.FoamFileError(f"{case_dir}: a case with cyclic patches runs with uniform alphaQGD / ScQGD (no alphaQGD or ScQGD field file)")
        # (QGDCoeffs varScModel7 on such a case is refused by foamfile.read_case_setup, by name)
        mesh = gmesh.unroll_cyclic(gmesh.cyclic_pairs)
        cells = mesh.array("cellGlobal")
        owned = np.arange(mesh.nCells) < n_global
    # this driver builds the block tables for a fixed-deltaT case with one GaussVolPoint stencil only: an adjustTimeStep case, which the library
    # can step on the blocks as well (QGD_FUSED_ADJUST, include/qgd_amd.h qgd_case_fused_info), runs the separate kernels here
    # (the blocks serve the explicit branch's one-launch step, shards included, and the implicitDiffusion branch's assembly of the U systems on one rank)
    # (a case with species steps with the separate kernels, on either branch: its species block reads the mass flux of every face)
    eligible = (not (opt.get("adjustTimeStep") or opt.get("termStencils") or species) and opt["stencil"] == "GaussVolPoint"
                and not (opt.get("implicitDiffusion") and world > 1))
    dev = Device(mesh, device_id, fv_schemes={"fvsc": {"default": opt["stencil"]}}, fused_tables=eligible)
    case = QGDFoamCase(dev, default_options(**opt))
    # value lists of fixedValue entries follow the device mesh's patch faces (a shard's through faceGlobal, the copies behind cyclic halves
    # take their originals' values); the case files keep theirs for the writer
    ff.apply_bcs(case, gmesh, mesh, bcs)
    if "alphaQGD" in fields or "ScQGD" in fields:
        # non-uniform alphaQGD / ScQGD files: cell values follow the relabelling; boundary faces keep their labels under
        # renumbering, a shard's real patch faces are found through faceGlobal (cut faces carry no patch value)
        nif_g = gmesh.nInternalFaces
        if world > 1:
            fg = mesh.array("faceGlobal")[mesh.nInternalFaces:]
            gb = np.where(fg >= nif_g, fg - nif_g, -1)
        else:
            gb = np.arange(gmesh.nBoundaryFaces)

        def local(pair):
            if pair is None:
                return None
            cellv, bndv = pair
            b = np.where(gb >= 0, bndv[np.maximum(gb, 0)], cellv[cells][mesh.array("owner")[mesh.nInternalFaces:]])
            return cellv[cells], b
        case.set_qgd_coeffs(alphaQGD=local(fields.get("alphaQGD")), ScQGD=local(fields.get("ScQGD")))
    var_sc = opt.get("varSc")
    if var_sc:
        # QGDCoeffs varScModel7: the sensor runs on the device, over the owned cells of a shard; the cells of constScCellSet follow the
        # relabelling and the cut (a shard marks those of them it holds)
        cs = var_sc["const_cells"]
        local_cells = np.nonzero(np.isin(cells, cs))[0].astype(np.int32) if cs is not None else None
        case.set_var_sc(**dict(var_sc, const_cells=local_cells))
    if species:
        # the species block of reactingLagrangianQGDFoam, passive: the Y_i advance with the flow on the device (QGDFoamCase.set_species)
        # (shards and cyclic patches: ghost cells carry their originals' composition, which travels in the state message)
        ff.apply_species(case, species, cells, **({"halo": True} if species_halo else {}))
    case.set_fields(fields["U"][cells], fields["T"][cells], fields["p"][cells])
    adjust = bool(case.options.adjustTimeStep)
    if world > 1:
        case.set_stream(torch.cuda.current_stream().cuda_stream)
        if staged:
            class Halo(HostStaged, RangeHalo):
                pass
            Halo.torch = torch
            halo = Halo(case, rank, world, dist, alloc=lambda c: torch.empty(c, dtype=torch.float64), arg=None)
        else:
            halo = RangeHalo(case, rank, world, dist, alloc=lambda c: torch.empty(c, dtype=torch.float64, device="cuda"),
                             arg=lambda t: t.data_ptr())
        from .halo import allreduce_max_of
        allreduce_max = allreduce_max_of(torch, dist, case, staged)
        stepper = None
        if case.options.implicitDiffusion:
            # the reference's default branch on shards: phases 20..35 with their messages and all-reduced solver scalars
            # (include/qgd_amd.h "the implicitDiffusion branch on a cell-range shard")
            import ctypes as C
            from . import _lib as L
            from .halo import DistWorld, ImplicitShard, ImplicitStepper, device_tensor
            peers = [int(p) for p in mesh.array("haloPeer")]
            if staged:
                def to_t(ptr, cnt):
                    return torch.from_numpy(dev.to_host(ptr, (int(cnt),)))

                def from_t(t, ptr):
                    a = np.ascontiguousarray(t.numpy())
                    if a.nbytes:
                        L.check(L.lib.qgd_device_copy(dev._h, C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, 1), "qgd_device_copy")
            else:
                to_t = lambda ptr, cnt: device_tensor(torch, ptr, cnt)     # noqa: E731  (views of the library's buffers)
                from_t = lambda t, ptr: None                               # noqa: E731
            stepper = ImplicitStepper(DistWorld(ImplicitShard(case), dist, torch, peers, to_t, from_t, kinds=range(5), device_reduce=not staged))
        else:
            halo.exchange()

    # functions{} of system/controlDict: probes, fieldMinMax, qgdIntegrals, qgdPatchFluxes -- and, in a case with species, species names in
    # the fields of the first two, qgdSpeciesIntegrals and qgdSpeciesPatchFluxes -- through one device monitor (monitor.py), sampled
    # after the steps at which one of them is due and read two samples late.  On several ranks every rank samples its shard and the
    # parts are combined on rank 0 (monitor.combine) -- a combination that has not run on more than one GPU yet.
    functions = None
    func_specs = ff.read_functions(cd, warn=log, species=species["names"] if species else None)
    if func_specs:
        from .monitor import FunctionObjects
        if world > 1:
            cg = mesh.array("cellGlobal")
            where = {int(cg[i]): int(i) for i in np.nonzero(owned)[0]}
            local_of = lambda g: where.get(g, -1)     # noqa: E731

            def gather_parts(sample):
                parts = [None] * world
                dist.all_gather_object(parts, sample)
                return parts
        else:
            local_of, gather_parts = (lambda g: g), None
        functions = FunctionObjects(case, func_specs, gmesh, case_dir, t0_name, local_of, old_of_new, is_root=rank == 0,
                                    gather=gather_parts, log=log, species=species["names"] if species else None)

    def advance_plain(n):
        if world == 1:
            case.step(n)
            return
        if stepper is not None:
            stepper.step(n, (lambda: allreduce_max(case)) if adjust else None)
        else:
            for _ in range(n):
                halo.step(allreduce_max if adjust else None)
        case.sync()

    def gather(name, local=None):
        """owned cells of every rank -> the field in the case's own cell order (rank 0; None elsewhere); local: this rank's values (default: the flow field `name`)"""
        local = case.field(name) if local is None else local
        if world == 1:
            out = np.empty((n_global,) + local.shape[1:])
            out[cells[owned]] = local[owned]     # (a mesh with cyclic patches carries copies of its cells behind the real ones)
            return out
        parts = [None] * world if rank == 0 else None
        dist.gather_object((cells[owned], local[owned]), parts, dst=0)
        if rank != 0:
            return None
        out = np.empty((n_global,) + local.shape[1:])
        for idx, vals in parts:
            out[idx] = vals
        return out

    dt, end_time, chunk, precision, total = apprun.run_control(cd, t0, n_steps, adjust, apprun.ADJUST_REFUSAL, run_time=not adjust)
    branch = "implicitDiffusion true" if opt.get("implicitDiffusion") else "explicit branch"
    log(f"QGDFoam (qgdsolver_amd, {branch}): {n_global} cells on {world} rank(s), fvsc {opt['stencil']}, "
        f"deltaT {dt:g}, start {t0_name}, cell order {renumber}")
    if species:
        log(f"  species {' '.join(species['names'])} (inert {species['inert']}): passive composition, one thermo, no chemistry")
        if opt.get("implicitDiffusion"):
            log(f"  species solves: tolerance {species['tolerance']:g}, maxIter {species['maxIter']}, {case.species_info()['batchWidth']} species per solve; "
                "they start from the old Y_i, as OpenFOAM's do")
    if opt.get("implicitDiffusion"):
        x = os.environ.get("QGD_IMPL_XEXTRAP", "3")
        if x != "0":
            log(f"  NOTE: the U and e solves start from the predictor + the correction of the last steps extrapolated in time (QGD_IMPL_XEXTRAP={x}; "
                + ("Lagrange weights from the deltaT ratios under adjustTimeStep; " if adjust else "")
                + "limited per value), not from the predictor alone as OpenFOAM does: same systems, same tolerance, same answer to that "
                "tolerance -- but the 'initial' residuals and iteration counts below are NOT comparable with a reference QGDFoam log.  "
                "QGD_IMPL_XEXTRAP=0 restores OpenFOAM's start values.")
    wall0 = _time.perf_counter()

    def report(done, t, info):
        if world > 1:
            mins = [None] * world
            dist.all_gather_object(mins, (info["minRho"], info["minE"], info["CoNum"]))
            info["minRho"], info["minE"] = min(m[0] for m in mins), min(m[1] for m in mins)
            info["CoNum"] = max(m[2] for m in mins)
        log(f"Time = {time_name(t, precision)}  steps {done}  deltaT {info['deltaT']:.6g}  Courant max {info['CoNum']:.6g}  "
            f"min rho {info['minRho']:.6g}  min e {info['minE']:.6g}  ClockTime {_time.perf_counter() - wall0:.2f} s")
        if opt.get("implicitDiffusion"):
            apprun.log_implicit_solves(log, case.implicit_info(), case.options)
        if species and opt.get("implicitDiffusion"):
            si = case.species_implicit_info()
            log("  " + "  ".join(f"{k}: {v['initial']:.3g} -> {v['final']:.3g} in {v['iterations']}" for k, v in si["species"].items()))
            if si["unconvergedSteps"]:
                log(f"  WARNING: {si['unconvergedSteps']} step(s) so far in which a species solve stopped above its tolerance "
                    f"(tolerance {species['tolerance']:g}, maxIter {species['maxIter']})")
            if si["stalledSteps"]:
                log(f"  NOTE: {si['stalledSteps']} step(s) so far in which a species solve ended at the rounding floor of its residual, above "
                    f"its tolerance {species['tolerance']:g}")
        if var_sc:
            sc_hi, sc_lo = case.sc_range()
            if world > 1:
                both = [None] * world
                dist.all_gather_object(both, (sc_hi, sc_lo))
                sc_hi, sc_lo = max(b[0] for b in both), min(b[1] for b in both)
            log(f"max/min ScQGD: {sc_hi:.6g}/{sc_lo:.6g}")     # [varScModel7.C L256-259]
        if not np.isfinite(info["minRho"]) or info["minRho"] <= 0:
            raise FloatingPointError(f"density lost positivity at time {t:g}")

    def write_time(name):
        data = {f: gather(f) for f in ("U", "T", "p", "rho") + (("ScQGD",) if var_sc else ())}
        if rank == 0:
            _write_cell_fields(case_dir, name, data, bcs, gmesh, var_sc)
        if species:
            # (gathered from the owned cells like the flow fields: the real cells only of a mesh with cyclic patches)
            Y = {sn: gather(sn, case.species_field(sn)) for sn in species["names"]}
            if rank == 0:
                ff.write_species_fields(case_dir, name, gmesh, species, Y)

    # (adjustTimeStep without -nSteps: total is None and the loop runs to endTime, the write cadence stays `chunk`)
    written = apprun.step_chunks(case, apprun.stepping(advance_plain, functions, t0), t0, chunk, total, precision, report, write_time if write else None,
                                 end_time)
    if functions is not None:
        functions.finish()
    log("End")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return dev, case, written


def main(argv=None):
    return apprun.main("QGDFoam", __doc__, run, argv=argv, extra_args=(
        ("-renumber", dict(dest="renumber", default="none", choices=["none", "rcm", "morton"],
                           help="relabel the cells on the device side (results are written in the case's own order)")),
        ("-backend", dict(dest="backend", default="nccl", choices=["nccl", "gloo"],
                          help="multi-rank transport; gloo = host-staged messages, all ranks on GPU 0 (debugging)"))))


if __name__ == "__main__":
    sys.exit(main())
