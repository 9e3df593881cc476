"""A/B of the C3 apply in one process: ho_block_z 2 (default), ho_block_z 4, ho_block_z 4 + ho_uniform 1,
alternated `rounds` times.  usage: ab_um.py LIB n rounds OUT.json"""
import json
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))
import numpy as np  # noqa: E402
import cdfem  # noqa: E402

lib, n, rounds, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
if lib != "-":
    cdfem.LIB_PATH = os.path.abspath(lib)
cdfem.lib()
p, iters, steps = 4, 20, 3
mesh = cdfem.box_mesh(3, (n, n, n), p, with_coords=False)
ctx = cdfem.Context(0)
b = np.random.default_rng(20261015).uniform(-1, 1, mesh.nl)
configs = [("bz2", {"ho_block_z": 2}), ("bz4", {"ho_block_z": 4}), ("bz4_um", {"ho_block_z": 4, "ho_uniform": 1})]
if len(sys.argv) > 5:
    configs = [c for c in configs if c[0] in sys.argv[5].split(",")]
res = {k: [] for k, _ in configs}
xs = {}
for rd in range(rounds):
    for name, opts in configs:
        try:
            for k, v in opts.items():
                ctx.set_option(k, v)
        except cdfem.CdfemError as e:
            print(name, "skipped:", e, flush=True)
            continue
        ctx.upload_mesh(mesh)
        ctx.set_structured(n, n, n)
        ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=(1.0, -2.0, 0.5), mass=1.0)
        _, B = ctx.form_linear_system(np.zeros(mesh.nl), b)
        dB = ctx.to_device(B)
        dX = ctx.alloc(8 * mesh.nl)

        def step():
            return ctx.solve_device(dB, dX, method="cg", pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=iters,
                                    check_every=iters)
        step()
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        ctx.synchronize()
        dt = (time.perf_counter() - t0) / steps
        ctx.set_option("profile_mask", 1 << cdfem.K_APPLY)
        ctx.profile(True)
        step()
        ctx.synchronize()
        each = np.asarray(ctx.profile_launches(cdfem.K_APPLY))
        ctx.profile(False)
        ctx.set_option("profile_mask", -1)
        full = each[each >= 0.5 * np.median(each)]
        rec = {"kernel": ctx.kernel_name(cdfem.K_APPLY), "ms_per_step": dt * 1e3,
               "dof_iter_per_s": mesh.nl * iters / dt, "apply_us": float(full.mean()) * 1e3,
               "apply_us_min": float(full.min()) * 1e3, "bytes": ctx.kernel_bytes(cdfem.K_APPLY),
               "flops": ctx.kernel_flops(cdfem.K_APPLY)}
        rec["hbm_frac"] = rec["bytes"] / (rec["apply_us"] * 1e-6) / 8e12
        rec["tflops"] = rec["flops"] / (rec["apply_us"] * 1e-6) / 1e12
        res[name].append(rec)
        print(rd, name, json.dumps(rec), flush=True)
        if rd == 0 and mesh.nl < 40e6:
            xs[name] = ctx.from_device(dX, mesh.nl)
        for k in opts:
            ctx.set_option(k, 2 if k == "ho_block_z" else 0)
        ctx.free(dB)
        ctx.free(dX)
if xs.get("bz4") is not None and xs.get("bz4_um") is not None:
    res["um_vs_bz4_rel"] = float(np.linalg.norm(xs["bz4_um"] - xs["bz4"]) / np.linalg.norm(xs["bz4"]))
    print("um vs bz4:", res["um_vs_bz4_rel"])
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
ctx.close()
