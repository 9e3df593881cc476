"""Prints kernel_name, kernel_flops and kernel_bytes (repr of the doubles, or the refusal's text) of every
kernel id over the configurations the cost model distinguishes.  Run once per library and diff the outputs:

    python profiles/r15/refactor_capi/cost_model.py [--lib PATH/libcdfem.so] > OUT
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "continuum-mechanics-mfem_amd", "python"))
import cdfem  # noqa: E402
from oracle import oracle as O  # noqa: E402

C3 = (1.0, -2.0, 0.5)
DEFAULTS = dict(pa_uniform=1, pa_affine=2, pa_geom=0, ho_brick=1, ho_uniform=0, ho_block_z=2, ho_geom=0, gm_pb=1,
                sell_order=8, spmv_lds=-1)


def report(ctx, label):
    for k in range(5):
        row = []
        for f in (ctx.kernel_name, ctx.kernel_flops, ctx.kernel_bytes):
            try:
                row.append(repr(f(k)))
            except cdfem.CdfemError as e:
                row.append(str(e))
        print(f"{label} | id {k} | " + " | ".join(row))


def box(ctx, label, dim, shape, p, pert=0.0, structured=True, kinds=7, solve=None, **opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    om = O.BoxMesh(dim, shape, p, perturb=pert)
    ctx.upload_mesh(cdfem.Mesh(dim, p, om.verts, om.dofmap, om.nl, om.ess))
    if structured:
        ctx.set_structured(*shape)
    ctx.pa_setup(kinds=kinds, kappa=0.1, alpha=1.0, conv=C3[:dim], mass=1.0)
    if solve:
        B = np.random.default_rng(1).uniform(-1, 1, om.nl)
        B[om.ess] = 0.0
        ctx.solve(B, method=solve, pc="jacobi", rel_tol=0.0, abs_tol=0.0, max_iter=3)
    report(ctx, label + " " + " ".join(f"{k}={v}" for k, v in opts.items()))
    for k in opts:
        ctx.set_option(k, DEFAULTS[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    if args.lib:
        cdfem.LIB_PATH = os.path.abspath(args.lib)
    with cdfem.Context(0) as ctx:
        for kinds in (7, 5):
            for un in (1, 0):
                for af in (2, 1, 0):
                    box(ctx, f"p2 box 8^3 kinds {kinds}", 3, (8, 8, 8), 2, kinds=kinds, pa_uniform=un, pa_affine=af)
        box(ctx, "p2 box 8^3 jacobi cg (class table)", 3, (8, 8, 8), 2, solve="cg")
        box(ctx, "p2 perturbed structured 9x6x7", 3, (9, 6, 7), 2, pert=0.1, pa_geom=1)
        box(ctx, "p2 perturbed unstructured 5x6x7", 3, (5, 6, 7), 2, pert=0.1, structured=False, pa_geom=1)
        for hb in (1, 0):
            box(ctx, "p4 box 4^3", 3, (4, 4, 4), 4, ho_brick=hb)
        box(ctx, "p4 box 4^3", 3, (4, 4, 4), 4, ho_block_z=4, ho_uniform=1)
        box(ctx, "p4 perturbed structured 4^3", 3, (4, 4, 4), 4, pert=0.1, ho_geom=1)
        box(ctx, "p4 perturbed unstructured 3x4x5", 3, (3, 4, 5), 4, pert=0.1, structured=False, ho_geom=1)
        box(ctx, "p2 unstructured hex 5x6x7", 3, (5, 6, 7), 2, pert=0.1, structured=False)
        box(ctx, "p1 unstructured hex 5x6x7 kinds 3", 3, (5, 6, 7), 1, pert=0.1, structured=False, kinds=3)
        box(ctx, "2D p2 6x6", 2, 6, 2, structured=False)
        for order, lds in ((8, -1), (8, 0), (6, 64)):
            ctx.set_option("sell_order", order)
            ctx.set_option("spmv_lds", lds)
            ctx.upload_mesh(cdfem.kuhn_mesh(3, 4, 2))
            ctx.fa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=C3, mass=1.0)
            report(ctx, f"tets 4^3 x 6 P2 sell_order={order} spmv_lds={lds}")
        ctx.set_option("sell_order", 8)
        ctx.set_option("spmv_lds", -1)
        for pb in (1, 0):
            box(ctx, "p2 box 8^3 after bicgstab", 3, (8, 8, 8), 2, solve="bicgstab", gm_pb=pb)


if __name__ == "__main__":
    main()
