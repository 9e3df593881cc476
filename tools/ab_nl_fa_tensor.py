"""The assembled tensor Jacobian (cdfem_nl_fa_setup) beside the matrix-free one (cdfem_nl_pa_setup), in one process
(GPU box only).

Meshes (--cases, all in the one process): hexN_pP, a perturbed (0.1) N^3 hex box at order P (P = 1, 2), and
quadN_pP, an unperturbed N^2 quad box at P = 1..3.  Default: hex64_p1 hex64_p2 quad1024_p1 quad1024_p2.  Set A's
coefficients (a0 = 1, a1 = 0.5, m0 = 1, m1 = 0.5) with dt = 0.1 on hexes and dt = 1e-4 on quads (at h = 1 / 1024 and
dt = 0.1 GMRES(30) + Jacobi does not converge on either path within thousands of iterations, and there would be
nothing to compare).  The reference driver's set-up: essential dofs on x = 1, the Neumann flux 0.25 on x = 0 through
cdfem_bdr_set / cdfem_bdr_lf_assemble.  Two contexts on the same mesh, neither declared structured: `fa` after
cdfem_nl_fa_setup, `mf` after cdfem_nl_pa_setup, both linearised at the same smooth u.
  rebuild  after a warm-up round, R rounds of K cdfem_nl_gradient calls on a device vector.  Events: the HIP event
           pairs of CDFEM_K_NL_ASSEMBLE (k_nl_tensor_point + k_nl_tensor_elem), CDFEM_K_FA_GATHER (k_fa_gather +
           k_fa_eliminate) and CDFEM_K_SELL_FILL, microseconds per rebuild; wall: a host clock around the K calls,
           profiling off (each call ends in a synchronise).  The first call is recorded apart (the host pattern
           and the SpMV plan are cdfem_nl_fa_setup's, not timed here).
  apply    the same rounds interleave the two constrained Mults on device vectors, K back-to-back calls ending in
           a synchronise: microseconds per call (matrix-free: k_nl_tensor + E->L).
  break-even  Krylov iterations per rebuild above which assembling pays: rebuild wall time / (matrix-free apply -
           SpMV); null where the SpMV is not the faster apply.
  newton   three backward-Euler steps (u_old <- u on the device), Newton rel_tol 1e-7, GMRES(30) to 1e-8 from a
           zero guess: `fa` + Jacobi against `mf` + Jacobi, and on quad meshes `fa` + ILU(0) (the hex box's ILU
           sweep is launch-bound: one launch per level); Newton iterations per step, linear iterations,
           wall seconds of the three steps, median of --newton-rounds after one warm-up solve.

    python tools/ab_nl_fa_tensor.py [--cases hex64_p2 ...] [--rounds 5] [--calls 10] [--newton-rounds 3] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["hex64_p1", "hex64_p2", "quad1024_p1", "quad1024_p2"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=10, help="calls per window")
ap.add_argument("--newton-rounds", type=int, default=3)
ap.add_argument("--ilu-max-iter", type=int, default=200, help="cap of one GMRES + ILU(0) solve")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import cdfem  # noqa: E402

R, K = args.rounds, args.calls
FLUX = 0.25


def spread(a, nd=2):
    a = np.asarray(a, dtype=float)
    return dict(median=round(float(np.median(a)), nd), min=round(float(a.min()), nd), max=round(float(a.max()), nd))


def clock(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def run_case(case):
    m = re.fullmatch(r"(hex|quad)(\d+)_p(\d)", case)
    if not m:
        raise SystemExit("--cases: hexN_pP or quadN_pP")
    dim, n, p = (3 if m.group(1) == "hex" else 2), int(m.group(2)), int(m.group(3))
    pert = 0.1 if dim == 3 else 0.0
    coeffs = dict(dt=0.1 if dim == 3 else 1e-4, a0=1.0, a1=0.5, m0=1.0, m1=0.5, u_ref=0.0)

    def note(msg):
        print(f"[{case}] {msg}", file=sys.stderr, flush=True)

    mesh = cdfem.box_mesh(dim, n, p, perturb=pert)
    xyz = mesh.dof_xyz
    mesh.ess = np.nonzero(xyz[:, 0] == 1.0)[0].astype(np.int32)            # essential on x = 1
    fe = np.nonzero(np.all(mesh.verts[:, 0::2, 0] == 0.0, axis=1))[0].astype(np.int32)  # elements on x = 0
    ff = np.zeros(len(fe), dtype=np.int32)                                 # local facet 2 * 0 + 0
    u_old = 1.0 + 0.5 * np.sin(np.pi * xyz[:, 0]) * np.cos(np.pi * xyz[:, 1])
    u = u_old + 0.3 * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, -1])
    v = np.random.default_rng(20261021).uniform(-1.0, 1.0, mesh.nl)

    fa = cdfem.Context(0).upload_mesh(mesh)
    mf = cdfem.Context(0).upload_mesh(mesh)
    ctxs = dict(fa=fa, mf=mf)
    fa.nl_fa_setup(**coeffs)
    mf.nl_pa_setup(**coeffs)
    g = None
    for c in ctxs.values():
        c.nl_set_old(u_old)
        c.bdr_set(fe, ff)
        g = c.bdr_lf_assemble(np.full((len(fe), c.bdr_rule_size()), FLUX))
        c.nl_set_rhs(g)
    dev = {k: dict(u=c.to_device(u), v=c.to_device(v), y=c.alloc(8 * mesh.nl), w=c.to_device(u_old)) for k, c in ctxs.items()}

    def gradient(k):
        c = ctxs[k]
        c._chk(c.L.cdfem_nl_gradient(c.h, C.c_void_p(dev[k]["u"]), cdfem.DEVICE))

    first = {k: round(clock(lambda: gradient(k)) * 1e3, 2) for k in ctxs}
    nnz = len(fa.fa_csr()[1])
    note(f"first nl_gradient ms {first}, nnz {nnz}")

    slots = dict(element=cdfem.K_NL_ASSEMBLE, gather_eliminate=cdfem.K_FA_GATHER, sell_fill=cdfem.K_SELL_FILL)
    ev = {k: [] for k in slots}
    rebuild_wall, apply_wall = [], {k: [] for k in ctxs}
    for rnd in range(R + 1):
        fa.profile(True)
        for _ in range(K):
            gradient("fa")
        got = {k: fa.profile_read(s) for k, s in slots.items()}
        fa.profile(False)
        assert all(cnt == K for _, cnt in got.values()), got
        tw = clock(lambda: [gradient("fa") for _ in range(K)])
        ta = {}
        for k, c in ctxs.items():
            c.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                c.mult_device(dev[k]["v"], dev[k]["y"], constrained=True)
            c.synchronize()
            ta[k] = time.perf_counter() - t0
        if rnd:  # round 0 is the warm-up
            for k, (ms, cnt) in got.items():
                ev[k].append(ms * 1e3 / cnt)
            rebuild_wall.append(tw * 1e6 / K)
            for k in ctxs:
                apply_wall[k].append(ta[k] * 1e6 / K)
    rec = {"case": case, "dim": dim, "n": n, "p": p, "perturb": pert, "dt": coeffs["dt"], "ne": int(mesh.ne),
           "nl": int(mesh.nl), "nnz": int(nnz), "neumann_facets": int(len(fe)), "essential_dofs": int(len(mesh.ess)),
           "rounds": R, "calls_per_window": K, "first_nl_gradient_ms": first,
           "rebuild_us_events": {k: spread(a) for k, a in ev.items()},
           "rebuild_us_wall": spread(rebuild_wall),
           "apply_us_wall": {k: spread(a) for k, a in apply_wall.items()},
           "apply_kernel": {k: c.kernel_name(cdfem.K_APPLY) for k, c in ctxs.items()}}
    gain = rec["apply_us_wall"]["mf"]["median"] - rec["apply_us_wall"]["fa"]["median"]
    rec["apply_fa_over_mf"] = round(rec["apply_us_wall"]["fa"]["median"] / rec["apply_us_wall"]["mf"]["median"], 3)
    rec["break_even_iterations_per_rebuild"] = round(rec["rebuild_us_wall"]["median"] / gain, 1) if gain > 0 else None
    note(f"rebuild {rec['rebuild_us_wall']} events {rec['rebuild_us_events']} apply {rec['apply_us_wall']} "
         f"break-even {rec['break_even_iterations_per_rebuild']}")

    # three backward-Euler steps, u_old <- u on the device
    kw = dict(rel_tol=1e-7, max_iter=8, method="gmres", lin_rel_tol=1e-8, lin_abs_tol=0.0)
    legs = [("fa_jacobi", "fa", "jacobi", 4000), ("mf_jacobi", "mf", "jacobi", 4000)]
    if dim == 2:
        legs.append(("fa_ilu", "fa", "ilu", args.ilu_max_iter))

    def three_steps(k, pc, lin_max_iter):
        c, d = ctxs[k], dev[k]
        c._chk(c.L.cdfem_memcpy(c.h, C.c_void_p(d["y"]), cdfem.DEVICE, C.c_void_p(d["w"]), cdfem.DEVICE, 8 * mesh.nl))
        out = []
        for _ in range(3):
            c.nl_set_old(d["y"], where=cdfem.DEVICE)
            info, hist = c.newton_solve_device(d["y"], pc=pc, lin_max_iter=lin_max_iter, **kw)
            out.append((info, hist))
            if not info["converged"]:
                break
        return out

    newton = {}
    for name, k, pc, cap in legs:
        c = ctxs[k]
        c.nl_set_old(dev[k]["w"], where=cdfem.DEVICE)
        c.newton_solve_device(dev[k]["u"], pc=pc, lin_max_iter=min(cap, 40), **dict(kw, max_iter=1))  # warm-up
        c._chk(c.L.cdfem_memcpy(c.h, C.c_void_p(dev[k]["u"]), cdfem.DEVICE, u.ctypes.data, cdfem.HOST, 8 * mesh.nl))
        secs, runs = [], None
        for _ in range(args.newton_rounds):
            t0 = time.perf_counter()
            runs = three_steps(k, pc, cap)
            secs.append(time.perf_counter() - t0)
        newton[name] = dict(converged=bool(all(i["converged"] for i, _ in runs) and len(runs) == 3),
                            newton_iterations=[int(i["iterations"]) for i, _ in runs],
                            linear_iterations=[int(i["linear_iterations"]) for i, _ in runs],
                            seconds=spread(secs, 4),
                            residual_seconds=round(sum(i["residual_seconds"] for i, _ in runs), 5),
                            jacobian_seconds=round(sum(i["jacobian_seconds"] for i, _ in runs), 5),
                            linear_seconds=round(sum(i["linear_seconds"] for i, _ in runs), 5),
                            final_residual=float(runs[-1][1]["residual"][-1]))
        newton[name]["u_final"] = c.from_device(dev[k]["y"], mesh.nl)
        note(f"{name}: { {a: b for a, b in newton[name].items() if a != 'u_final'} }")
    ref = newton["mf_jacobi"].pop("u_final")
    for name in list(newton):
        if "u_final" in newton[name]:
            uf = newton[name].pop("u_final")
            newton[name]["rel_l2_against_mf_jacobi"] = float(np.linalg.norm(uf - ref) / np.linalg.norm(ref))
    rec["newton_three_steps"] = newton
    for k, c in ctxs.items():
        for ptr in dev[k].values():
            c.free(ptr)
        c.close()
    return rec


records = []
for case in args.cases:
    records.append(run_case(case))
    text = json.dumps(records, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fo:
            fo.write(text + "\n")
print(json.dumps(records, indent=1))
