"""BiCGStab against GMRES(30) on one context, alternating in one process (GPU box only).

System: C2's (64^3 hex, p = 2, D + C + M, Jacobi, the bench's RHS seed), optionally its perturbed box
(perturb 0.1, pa_geom 1) and C4's (Kuhn 55^3 P2, assembled).  After a warm-up round, R rounds alternate
the two solvers:
  (a) fixed work: GMRES(30) for 60 steps and BiCGStab for 30 iterations (60 operator applies each),
      rtol = atol = 0; wall time from a host clock around a device synchronise, us per apply-equivalent
      with the spread over rounds; with HIP events on, the K_APPLY / K_UPDATE (GMRES: K_ORTH) times;
  (b) to tolerance: both to rtol 1e-10 / atol 1e-12; iterations, applies, seconds and the true
      preconditioned residual of each result, computed with ctx.mult.
The read16 / copy16 stream probes run in the same process.

    python tools/ab_bicgstab.py [--rounds R] [--n 64] [--systems c2,c2pert,c4] [--json out.json]
    python tools/ab_bicgstab.py --trace-run            # the solves alone, for rocprofv3 --kernel-trace
    python tools/ab_bicgstab.py --stats DIR [--n 64]   # k_bcgs_* averages of that trace and their TB/s
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--n4", type=int, default=55, help="cubes per edge of the Kuhn mesh (c4)")
ap.add_argument("--systems", default="c2,c2pert")
ap.add_argument("--json", default=None)
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--stats", default=None, help="rocprofv3 output directory (searched for *kernel_trace.csv)")
args = ap.parse_args()
C3 = (1.0, -2.0, 0.5)
SEED = 20261015


def vector_kernel_bytes(nl, nbrick, patch):
    """Algorithmic bytes per launch of the five vector kernels (Jacobi), from shapes: the sum is
    cdfem_kernel_bytes(CDFEM_K_UPDATE) after a BiCGStab solve."""
    src = 8.0 * 9 ** 3 * nbrick + nl if patch else 8.0 * nl
    vt = 8.0 * nl * 3 + src
    return {"k_bcgs_p": 8.0 * nl * 4, "k_bcgs_v": vt, "k_bcgs_s": 8.0 * nl * 3, "k_bcgs_t": vt,
            "k_bcgs_x": 8.0 * nl * 7}


if args.stats:
    files = glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {args.stats}")
    dur = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0].replace("void ", "").replace("cdfem::", "").strip()
            dur.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    n = args.n
    nl, nbrick = (2 * n + 1) ** 3, ((n + 3) // 4) ** 3
    by = vector_kernel_bytes(nl, nbrick, True)
    print("kernel,launches,avg_us,median_us,bytes,TBps,share_of_8TBps")
    for name in sorted(dur):
        if not (name.startswith("k_bcgs") or name.startswith("k_gm_") or name.startswith("k_brick")):
            continue
        d = np.array(dur[name]) / 1e3
        full = d[d >= 0.5 * np.median(d)]  # launches past the stop exit at entry
        b = by.get(name.split("<")[0])
        tb = b / (full.mean() * 1e-6) / 1e12 if b else float("nan")
        print(f"{name},{len(d)},{full.mean():.2f},{np.median(d):.2f},{b or 0:.0f},{tb:.3f},{tb / 8.0:.3f}")
    raise SystemExit(0)

import cdfem  # noqa: E402


def setup(ctx, system):
    if system == "c4":
        mesh = cdfem.kuhn_mesh(3, args.n4, 2, with_coords=False)
        ctx.upload_mesh(mesh)
        ctx.fa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
        return mesh
    n = args.n
    pert = system == "c2pert"
    ctx.set_option("pa_geom", 1 if pert else 0)
    mesh = cdfem.box_mesh(3, n, 2, perturb=0.1 if pert else 0.0, with_coords=False)
    ctx.upload_mesh(mesh).set_structured(n, n, n)
    ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
    return mesh


SOLVERS = {"gmres": dict(method="gmres", restart=30, applies=1, fixed=60, update=cdfem.K_ORTH),
           "bicgstab": dict(method="bicgstab", restart=30, applies=2, fixed=30, update=cdfem.K_UPDATE)}


def spread(v):
    v = np.asarray(v, dtype=float)
    return dict(median=round(float(np.median(v)), 2), min=round(float(v.min()), 2), max=round(float(v.max()), 2))


def run(ctx, system):
    mesh = setup(ctx, system)
    b = np.random.default_rng(SEED).uniform(-1, 1, mesh.nl)
    _, B = ctx.form_linear_system(np.zeros(mesh.nl), b)
    dB, dX = ctx.to_device(B), ctx.alloc(8 * mesh.nl)
    dinv = None
    out = {"nl": int(mesh.nl)}
    if args.trace_run:
        for _ in range(3):
            for name, s in SOLVERS.items():
                ctx.solve_device(dB, dX, method=s["method"], pc="jacobi", max_iter=s["fixed"], restart=30,
                                 check_every=16)
        ctx.synchronize()
        return out
    fixed = {k: {"wall_us_per_apply": [], "apply_us": [], "update_us_per_apply": []} for k in SOLVERS}
    for prof in (False, True):
        for rnd in range(args.rounds + 1):
            for name, s in SOLVERS.items():
                ctx.set_option("profile_mask", (1 << cdfem.K_APPLY) | (1 << cdfem.K_E2L) | (1 << s["update"]))
                ctx.profile(prof)
                ctx.synchronize()
                t0 = time.perf_counter()
                info = ctx.solve_device(dB, dX, method=s["method"], pc="jacobi", max_iter=s["fixed"], restart=30,
                                        check_every=16)
                ctx.synchronize()
                dt = time.perf_counter() - t0
                assert info["iterations"] == s["fixed"]
                na = s["fixed"] * s["applies"]
                if prof:
                    a, e, u = (ctx.profile_read(k) for k in (cdfem.K_APPLY, cdfem.K_E2L, s["update"]))
                    ctx.profile(False)
                    if rnd:
                        fixed[name]["apply_us"].append((a[0] + e[0]) * 1e3 / na)
                        fixed[name]["update_us_per_apply"].append(u[0] * 1e3 / na)
                elif rnd:
                    fixed[name]["wall_us_per_apply"].append(dt * 1e6 / na)
    out["fixed"] = {k: {m: spread(v) for m, v in r.items()} for k, r in fixed.items()}
    out["update_bytes_per_iteration"] = None
    tol = {}
    for name, s in SOLVERS.items():
        ts = []
        for rnd in range(3):
            ctx.synchronize()
            t0 = time.perf_counter()
            info = ctx.solve_device(dB, dX, method=s["method"], pc="jacobi", rel_tol=1e-10, abs_tol=1e-12,
                                    max_iter=5000, restart=30, check_every=16)
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        if name == "bicgstab":
            out["update_bytes_per_iteration"] = ctx.kernel_bytes(cdfem.K_UPDATE)
            out["update_kernel"] = ctx.kernel_name(cdfem.K_UPDATE)
        x = ctx.from_device(dX, mesh.nl)
        if dinv is None:
            d = ctx.diagonal()
            ess = np.zeros(mesh.nl, dtype=bool)
            ess[mesh.ess] = True
            dinv = np.where(ess, 1.0, 1.0 / d)
        res = np.linalg.norm(dinv * (B - ctx.mult(x, constrained=True))) / np.linalg.norm(dinv * B)
        tol[name] = dict(converged=info["converged"], iterations=info["iterations"],
                         applies=info["iterations"] * s["applies"], seconds=round(min(ts), 6),
                         seconds_all=[round(t, 6) for t in ts], true_prec_residual=float(res))
    out["to_tolerance"] = tol
    ctx.free(dB)
    ctx.free(dX)
    return out


ctx = cdfem.Context(0)
record = {}
try:
    for system in args.systems.split(","):
        record[system] = run(ctx, system)
    if not args.trace_run:
        record["stream_GBps"] = {"read16": round(ctx.stream_bench(0), 1), "copy16": round(ctx.stream_bench(2), 1)}
finally:
    ctx.set_option("pa_geom", 0)
    ctx.close()
text = json.dumps(record, indent=1)
print(text)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fo:
        fo.write(text + "\n")
