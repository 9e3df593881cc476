"""Full assembly beside partial assembly on one quad / hex mesh, in one process (GPU box only).

Meshes (--case): hexN_pP, a perturbed (0.1) N^3 hex box at order P (P = 1, 2), and quadN_pP, an N^2 quad box at
P = 1..4.  Two contexts on the same mesh, neither declared structured, D + C + M with kappa 0.1, c = (1, -2, 0.5),
s = 1: `fa` after cdfem_fa_setup (the SELL SpMV), `pa` after cdfem_pa_setup (the element kernel and the E->L sum).
  setup    wall milliseconds of the first cdfem_fa_setup (host pattern and SpMV plan included), of R repeats (the
           pattern reused: element kernel, gather, elimination, SELL fill, one synchronise) and of cdfem_pa_setup;
           the ILU(0) factorisation as the first ILU solve's wall time less the second's.  Per kernel: run the
           same command under `rocprofv3 --kernel-trace --stats` and read k_tensor_elem, k_fa_gather, k_fa_eliminate,
           k_sell_fill and k_ilu_factor_level from its stats (profiles/r16/fa_tensor/).
  apply    after a warm-up round, R rounds interleave the two constrained Mults on device vectors: K back-to-back
           calls ending in a synchronise, microseconds per call (PA: apply + E->L), median [min, max];
           with cdfem_kernel_bytes of each.
  solves   GMRES(30) to rtol 1e-10 / atol 1e-12 from a zero guess, right-hand side of ones: PA + Jacobi,
           FA + Jacobi, FA + ILU(0): iterations and seconds (the solver's own clock), median of R.

    python tools/ab_fa_tensor.py --case hex64_p2 [--rounds 5] [--calls 20] [--json out.json] [--no-ilu] [--no-solves]
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))

ap = argparse.ArgumentParser()
ap.add_argument("--case", default="hex64_p2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="calls per wall-clock window")
ap.add_argument("--max-iter", type=int, default=5000)
ap.add_argument("--no-ilu", action="store_true")
ap.add_argument("--no-solves", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import cdfem  # noqa: E402

m = re.fullmatch(r"(hex|quad)(\d+)_p(\d)", args.case)
if not m:
    raise SystemExit("--case: hexN_pP or quadN_pP")
dim, n, p = (3 if m.group(1) == "hex" else 2), int(m.group(2)), int(m.group(3))
pert = 0.1 if dim == 3 else 0.0
mesh = cdfem.box_mesh(dim, n, p, perturb=pert, with_coords=False)
FORM = dict(kinds=7, kappa=0.1, alpha=1.0, conv=(1.0, -2.0, 0.5)[:dim], mass=1.0)
R, K = args.rounds, args.calls


def spread(a, nd=2):
    a = np.asarray(a, dtype=float)
    return dict(median=round(float(np.median(a)), nd), min=round(float(a.min()), nd), max=round(float(a.max()), nd))


def note(msg):
    print(f"[{args.case}] {msg}", file=sys.stderr, flush=True)


def clock(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


fa = cdfem.Context(0).upload_mesh(mesh)
pa = cdfem.Context(0).upload_mesh(mesh)
setup = {"fa_first_ms": round(clock(lambda: fa.fa_setup(**FORM)), 2)}
setup["fa_again_ms"] = spread([clock(lambda: fa.fa_setup(**FORM)) for _ in range(R)])
setup["pa_first_ms"] = round(clock(lambda: pa.pa_setup(**FORM)), 2)
setup["pa_again_ms"] = spread([clock(lambda: pa.pa_setup(**FORM)) for _ in range(R)])
nnz = len(fa.fa_csr()[1])
note(f"setup done: {setup}")

ctxs = dict(fa=fa, pa=pa)
v = np.random.default_rng(20261021).uniform(-1.0, 1.0, mesh.nl)
dev = {k: (c.to_device(v), c.alloc(8 * mesh.nl)) for k, c in ctxs.items()}
wall = {k: [] for k in ctxs}
for rnd in range(R + 1):
    for k, c in ctxs.items():
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            c.mult_device(dev[k][0], dev[k][1], constrained=True)
        c.synchronize()
        if rnd:  # round 0 is the warm-up
            wall[k].append((time.perf_counter() - t0) * 1e6 / K)
for k, c in ctxs.items():
    for ptr in dev[k]:
        c.free(ptr)

record = {"case": args.case, "dim": dim, "n": n, "p": p, "perturb": pert, "ne": int(mesh.ne), "nl": int(mesh.nl),
          "nnz": int(nnz), "nnz_per_row": round(nnz / mesh.nl, 2), "rounds": R, "calls_per_window": K, "setup": setup,
          "apply_us_wall": {k: spread(a) for k, a in wall.items()},
          "apply_kernel": {k: c.kernel_name(cdfem.K_APPLY) for k, c in ctxs.items()},
          "apply_bytes": {k: c.kernel_bytes(cdfem.K_APPLY) for k, c in ctxs.items()}}
record["apply_fa_over_pa"] = round(record["apply_us_wall"]["fa"]["median"] / record["apply_us_wall"]["pa"]["median"], 3)

note(f"applies done: fa/pa {record['apply_fa_over_pa']}")
if not args.no_solves:
    _, B = fa.form_linear_system(np.zeros(mesh.nl), np.ones(mesh.nl))
    kw = dict(method="gmres", restart=30, rel_tol=1e-10, abs_tol=1e-12, max_iter=args.max_iter)
    legs = [("pa_jacobi", pa, "jacobi"), ("fa_jacobi", fa, "jacobi")] + ([] if args.no_ilu else [("fa_ilu", fa, "ilu")])
    solves = {}
    for name, c, pc in legs:
        first = clock(lambda: c.solve(B, pc=pc, **kw))  # warm-up: Jacobi scale / ILU factors, solver buffers
        runs = [c.solve(B, pc=pc, **kw)[1] for _ in range(R)]
        solves[name] = dict(converged=bool(all(r["converged"] for r in runs)), iterations=int(runs[0]["iterations"]),
                            seconds=spread([r["seconds"] for r in runs], 5), first_call_ms=round(first, 2))
        if pc == "ilu":
            again = clock(lambda: c.solve(B, pc=pc, **kw))
            setup["ilu_factor_ms"] = round(first - again, 2)
        note(f"{name}: {solves[name]}")
    record["solves"] = solves
fa.close()
pa.close()

text = json.dumps(record, indent=1)
print(text)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fo:
        fo.write(text + "\n")
