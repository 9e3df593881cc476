"""cdfem_set_option through the Python binding on a context: each kind of row of the option table refuses
with the library's text (cdfem_last_error) and leaves the context usable, and brick_byte_limit 0 restores
the default bound.  The table itself is checked value by value on the host (tests/test_options.py)."""
import numpy as np
import pytest

import cdfem
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REFUSALS = [
    ("no_such_option", 1, "unknown option no_such_option"),                              # unknown key
    ("cg_xfold", 2, "cg_xfold must be 0 or 1"),                                          # a flag
    ("gm_poll", 65, "gm_poll must be 1..64"),                                            # a range
    ("ho_mfma", 2, "ho_mfma must be 0, 1, 3, 8, 9 or 15"),                               # a list
    ("spmv_lds", 100, "spmv_lds must be -1 (auto), 0 (off) or rows per window, a multiple of 64 up to 65536"),
]


def _box(gpu_ctx):
    shape, p = (8, 8, 8), 2
    om = O.BoxMesh(3, shape, p)
    gpu_ctx.upload_mesh(cdfem.Mesh(3, p, om.verts, om.dofmap, om.nl, om.ess)).set_structured(*shape)
    gpu_ctx.pa_setup(kinds=7, kappa=0.1, alpha=1.0, conv=(1.0, -2.0, 0.5), mass=1.0)
    return om


def test_refusals_keep_the_context_usable(gpu_ctx):
    om = _box(gpu_ctx)
    x = np.random.default_rng(2).uniform(-1, 1, om.nl)
    y0 = gpu_ctx.mult(x)
    for key, value, text in REFUSALS:
        with pytest.raises(cdfem.CdfemError) as e:
            gpu_ctx.set_option(key, value)
        assert e.value.code == cdfem.ERR_ARG
        assert str(e.value) == f"cdfem error {cdfem.ERR_ARG}: {text}"
        np.testing.assert_array_equal(gpu_ctx.mult(x), y0)  # usable, and nothing was switched
    assert gpu_ctx.kernel_name(cdfem.K_APPLY) == "k_brick_cg"


def test_brick_byte_limit_zero_restores_the_brick_path(gpu_ctx):
    _box(gpu_ctx)
    try:
        assert gpu_ctx.kernel_name(cdfem.K_APPLY) == "k_brick_cg"
        gpu_ctx.set_option("brick_byte_limit", 4096)  # below the box's vectors: the generic kernels
        assert gpu_ctx.kernel_name(cdfem.K_APPLY) == "k_apply3d"
    finally:
        gpu_ctx.set_option("brick_byte_limit", 0)     # 0: the default 2^31
    assert gpu_ctx.kernel_name(cdfem.K_APPLY) == "k_brick_cg"
