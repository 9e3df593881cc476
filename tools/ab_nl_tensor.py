"""The matrix-free nonlinear form's kernels beside the linear applies of the same mesh, in one process (GPU box only).

Mesh: a perturbed (perturb 0.1) n^3 hex box at p = 2, n = 64 by default, not declared structured, so that all
three operators run the same launch structure: an element kernel writing an E-vector, then k_e2l.  Three contexts:
  nl     cdfem_nl_pa_setup (set A's coefficients), J(u) at a smooth u: k_nl_tensor in its three modes;
  qdata  cdfem_pa_setup(D + C + M) with pa_geom 0: k_apply3d on the per-point qdata stream;
  geom   the same with pa_geom 1: k_apply3d forming the geometric factors in the apply.
After a warm-up round, R rounds interleave the five kernels.  Each is timed twice:
  events   cdfem_profile_*: a HIP event pair around the element kernel alone (CDFEM_K_APPLY, CDFEM_K_NL_RESIDUAL,
           CDFEM_K_DIAGONAL), us per launch; all five are plain launches between two recorded events, so each
           figure carries the same few us of event overhead;
  wall     a host clock around K back-to-back calls on device vectors ending in a synchronise, profiling off:
           us per call, the E->L sum (and for the residual k_nl_finish) included.
Then one Newton solve of set A (essential dofs on the box's boundary, GMRES(30) + Jacobi at 1e-8 linear tolerance)
with its residual / Jacobian / linear seconds and the linear iterations of every Newton iteration, and the jvp's
roofline fraction from cdfem_kernel_flops / cdfem_kernel_bytes against 78.6 TFLOP/s f64 and 8 TB/s.

    python tools/ab_nl_tensor.py [--n 64] [--rounds 5] [--calls 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--calls", type=int, default=20, help="calls per wall-clock window")
ap.add_argument("--json", default=None)
args = ap.parse_args()

import cdfem  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 78.6e12, 8.0e12
COEFFS = dict(dt=0.1, a0=1.0, a1=0.5, m0=1.0, m1=0.5, u_ref=0.0)
n = args.n
mesh = cdfem.box_mesh(3, n, 2, perturb=0.1)
xyz = mesh.dof_xyz
u_old = 1.0 + 0.5 * np.sin(np.pi * xyz[:, 0]) * np.cos(np.pi * xyz[:, 1])
u = u_old + 0.3 * np.cos(2.0 * xyz[:, 0] + xyz[:, 1]) * np.exp(0.5 * xyz[:, 2])
v = np.random.default_rng(20261021).uniform(-1.0, 1.0, mesh.nl)


def spread(a):
    a = np.asarray(a, dtype=float)
    return dict(median=round(float(np.median(a)), 2), min=round(float(a.min()), 2), max=round(float(a.max()), 2))


nl = cdfem.Context(0).upload_mesh(mesh)
nl.nl_pa_setup(**COEFFS)
nl.nl_set_old(u_old)
nl.nl_gradient(u)
lin = {}
for name, geom in (("qdata", 0), ("geom", 1)):
    c = cdfem.Context(0)
    c.set_option("pa_geom", geom)
    c.upload_mesh(mesh)
    c.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=(1.0, -2.0, 0.5), mass=1.0)
    lin[name] = c
ctxs = dict(nl=nl, **lin)
dev = {k: (c.to_device(v), c.alloc(8 * mesh.nl), c.to_device(u)) for k, c in ctxs.items()}


def call(kind):
    """one call of kernel `kind` on device vectors, no host wait"""
    if kind == "residual":
        du, dy = dev["nl"][2], dev["nl"][1]
        nl._chk(nl.L.cdfem_nl_residual(nl.h, C.c_void_p(du), C.c_void_p(dy), cdfem.DEVICE))
    elif kind == "diagonal":
        nl._chk(nl.L.cdfem_pa_diagonal(nl.h, C.c_void_p(dev["nl"][1]), cdfem.DEVICE))
    else:
        key = "nl" if kind == "jvp" else kind
        ctxs[key].mult_device(dev[key][0], dev[key][1], constrained=True)


KINDS = {"residual": ("nl", cdfem.K_NL_RESIDUAL), "jvp": ("nl", cdfem.K_APPLY), "diagonal": ("nl", cdfem.K_DIAGONAL),
         "qdata": ("qdata", cdfem.K_APPLY), "geom": ("geom", cdfem.K_APPLY)}
events = {k: [] for k in KINDS}
wall = {k: [] for k in KINDS}
for rnd in range(args.rounds + 1):
    for kind, (key, slot) in KINDS.items():
        c = ctxs[key]
        c.profile(True)
        for _ in range(args.calls):
            call(kind)
        c.synchronize()
        ms, cnt = c.profile_read(slot)
        c.profile(False)
        assert cnt == args.calls, (kind, cnt)
        c.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(kind)
        c.synchronize()
        dt = time.perf_counter() - t0
        if rnd:  # round 0 is the warm-up
            events[kind].append(ms * 1e3 / cnt)
            wall[kind].append(dt * 1e6 / args.calls)

record = {"n": n, "p": 2, "perturb": 0.1, "ne": int(mesh.ne), "nl": int(mesh.nl), "rounds": args.rounds,
          "calls_per_window": args.calls,
          "kernel_us_events": {k: spread(a) for k, a in events.items()},
          "call_us_wall": {k: spread(a) for k, a in wall.items()},
          "kernel_names": {k: ctxs[key].kernel_name(cdfem.K_APPLY) for k, (key, _) in KINDS.items()}}
flops, nbytes = nl.kernel_flops(cdfem.K_APPLY), nl.kernel_bytes(cdfem.K_APPLY)
t = record["kernel_us_events"]["jvp"]["median"] * 1e-6
floor = max(flops / PEAK_FLOPS, nbytes / PEAK_BYTES)
record["jvp_roofline"] = dict(flops=flops, bytes=nbytes, flops_floor_us=round(flops / PEAK_FLOPS * 1e6, 2),
                              bytes_floor_us=round(nbytes / PEAK_BYTES * 1e6, 2),
                              bound="flops" if flops / PEAK_FLOPS > nbytes / PEAK_BYTES else "bytes",
                              fraction=round(floor / t, 4), tflops=round(flops / t / 1e12, 2),
                              tbps=round(nbytes / t / 1e12, 3))
for k in ("qdata", "geom"):
    tk = record["kernel_us_events"][k]["median"] * 1e-6
    record.setdefault("linear_apply", {})[k] = dict(flops=lin[k].kernel_flops(cdfem.K_APPLY),
                                                    bytes=lin[k].kernel_bytes(cdfem.K_APPLY),
                                                    tbps=round(lin[k].kernel_bytes(cdfem.K_APPLY) / tk / 1e12, 3))
for k, c in ctxs.items():
    for p in dev[k]:
        c.free(p)
for c in lin.values():
    c.set_option("pa_geom", 0)
    c.close()
nl.close()

# one Newton solve of set A, essential dofs on the boundary
with cdfem.Context(0).upload_mesh(mesh) as ctx:
    ctx.nl_pa_setup(**COEFFS)
    ctx.nl_set_old(u_old)
    g = np.zeros(mesh.nl)
    g[xyz[:, 0] > 0.5] = 1e-6
    ctx.nl_set_rhs(g)
    kw = dict(rel_tol=1e-7, max_iter=6, method="gmres", pc="jacobi", lin_rel_tol=1e-8, lin_abs_tol=0.0, lin_max_iter=4000)
    ctx.newton_solve(u_old, **dict(kw, max_iter=1, lin_max_iter=60))  # warm-up
    t0 = time.perf_counter()
    _, info, hist = ctx.newton_solve(u_old, **kw)
    dt = time.perf_counter() - t0
    record["newton"] = dict(converged=info["converged"], iterations=info["iterations"], seconds=round(dt, 4),
                            residual_seconds=round(info["residual_seconds"], 5),
                            jacobian_seconds=round(info["jacobian_seconds"], 5),
                            linear_seconds=round(info["linear_seconds"], 5),
                            linear_iterations=[int(i) for i in hist["linear_iterations"]],
                            residual=[float(r) for r in hist["residual"]],
                            linear_us_per_iteration=round(info["linear_seconds"] * 1e6 / max(1, info["linear_iterations"]), 1))
text = json.dumps(record, indent=1)
print(text)
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as fo:
        fo.write(text + "\n")
