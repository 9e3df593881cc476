"""Interleaved in-process A/B of the geometry-in-the-apply form (pa_geom 1: point data formed from the
element's trilinear map, pa_core.hpp elem_apply3d<..., GEO>) against the per-point qdata stream
(pa_geom 0) on a PERTURBED C2 box (64^3 hex p = 2, no element a parallelepiped), kinds 7 and 5.  With
--option ho_geom --p 4 (or 3) the same A/B of the high-order tile apply's geometry mode (k_apply3d_tile,
mode bit 32) against its stream.

Two contexts per kinds mask (the option is read by pa_setup); per round each runs a fixed Jacobi-CG solve
(apply launch time from the profiling events) and a fixed GMRES(30) solve.  Prints medians, the apply's
bytes and flops, and the relative difference of the two contexts' iterates as one JSON record.

    python tools/ab_geom.py [--option pa_geom] [--p 2] [--rounds 5] [--iters 100] [--n 64] [--kinds 7,5]
                            [--out record.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))
import cdfem  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--option", default="pa_geom", choices=["pa_geom", "ho_geom"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--gmres-iters", type=int, default=60)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--p", type=int, default=2)
ap.add_argument("--perturb", type=float, default=0.1)
ap.add_argument("--kinds", default="7,5")
ap.add_argument("--out", default="")
args = ap.parse_args()

n = args.n
mesh = cdfem.box_mesh(3, n, args.p, perturb=args.perturb, with_coords=False)
b = np.random.default_rng(1).uniform(-1, 1, mesh.nl)


def rel(a, c):
    return float(np.linalg.norm(a - c) / np.linalg.norm(c))


def one_pass(kinds):
    runs = []
    for geom in (1, 0):
        ctx = cdfem.Context(0)
        ctx.set_option(args.option, geom)
        ctx.upload_mesh(mesh).set_structured(n, n, n)
        ctx.pa_setup(kinds=kinds, kappa=0.1, conv=(1.0, -2.0, 0.5), mass=1.0)
        _, B = ctx.form_linear_system(np.zeros(mesh.nl), b)
        runs.append(dict(label=f"{args.option}={geom}", name=ctx.kernel_name(cdfem.K_APPLY), ctx=ctx,
                         dB=ctx.to_device(B), dX=ctx.alloc(8 * mesh.nl),
                         bytes=ctx.kernel_bytes(cdfem.K_APPLY), flops=ctx.kernel_flops(cdfem.K_APPLY),
                         cg_us=[], apply_us=[], upd_us=[], gm_us=[]))
    for rnd in range(args.rounds + 1):  # (round 0 warms up)
        for r in runs:
            ctx = r["ctx"]
            ctx.profile(True)
            ctx.synchronize()
            t0 = time.perf_counter()
            info = ctx.solve_device(r["dB"], r["dX"], method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0,
                                    max_iter=args.iters)
            ctx.synchronize()
            dt = time.perf_counter() - t0
            a = ctx.profile_read(cdfem.K_APPLY)
            u = ctx.profile_read(cdfem.K_UPDATE)
            ctx.profile(False)
            r["x_cg"] = ctx.from_device(r["dX"], mesh.nl)
            ctx.synchronize()
            t1 = time.perf_counter()
            ig = ctx.solve_device(r["dB"], r["dX"], method="gmres", pc="jacobi", rel_tol=0.0, abs_tol=0.0,
                                  max_iter=args.gmres_iters, restart=30)
            ctx.synchronize()
            dg = time.perf_counter() - t1
            r["x_gm"] = ctx.from_device(r["dX"], mesh.nl)
            if rnd:
                r["cg_us"].append(dt / info["iterations"] * 1e6)
                r["apply_us"].append(a[0] / max(a[1], 1) * 1e3)
                r["upd_us"].append(u[0] / max(u[1], 1) * 1e3)
                r["gm_us"].append(dg / ig["iterations"] * 1e6)
    out = {"rel_diff_cg_1_vs_0": rel(runs[0]["x_cg"], runs[1]["x_cg"]),
           "rel_diff_gmres_1_vs_0": rel(runs[0]["x_gm"], runs[1]["x_gm"])}
    for r in runs:
        med = {k: float(np.median(r[k])) for k in ("cg_us", "apply_us", "upd_us", "gm_us")}
        med["apply_us_min"] = float(np.min(r["apply_us"]))
        med["apply_kernel"] = r["name"]
        med["apply_bytes"] = r["bytes"]
        med["apply_flops"] = r["flops"]
        med["apply_gb_per_s"] = r["bytes"] / (med["apply_us"] * 1e-6) / 1e9
        med["apply_gflop_per_s"] = r["flops"] / (med["apply_us"] * 1e-6) / 1e9
        med["cg_dof_iter_per_s"] = mesh.nl / (med["cg_us"] * 1e-6)
        med["gmres_dof_iter_per_s"] = mesh.nl / (med["gm_us"] * 1e-6)
        out[r["label"]] = med
        r["ctx"].close()
    return out


rec = {"option": args.option, "shape": [n, n, n], "p": args.p, "perturb": args.perturb, "dofs": mesh.nl,
       "rounds": args.rounds, "cg_iters": args.iters, "gmres_iters": args.gmres_iters}
for k in [int(s) for s in args.kinds.split(",")]:
    rec[f"kinds={k}"] = one_pass(k)
text = json.dumps(rec, indent=1)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
