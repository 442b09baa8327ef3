"""
One batch gradient call and one batch Newton solve on the same handle for a counter run of its own (tools/README.md):
SSY 5^4 (or `ssy10`), B = 256.  The counters of batch_adjoint_kernel and batch_newton_kernel, divided by the
applications printed here, are instructions per application of the two kernels.

    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_SALU SQ_WAVE_CYCLES \
        --output-format csv -d OUT -- python tools/batch_gradient_pmc_run.py [ssy10]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdfs_via_autodiff_amd as S                       # noqa: E402
from batch_family import member, package_model         # noqa: E402

shapes = (10,) * 4 if "ssy10" in sys.argv[1:] else (5,) * 4
models = [package_model(S, "ssy", member("ssy", b)) for b in range(256)]
op = S.BatchOperator.from_models(models, shapes)
w, n_iter, err, status, n_apply = op.solve(np.full((256,) + shapes, 800.0), tol=1e-7, algorithm="newton", inner_rtol=1e-5,
                                           inner_atol=0.0)
print("newton: applications sum", int(n_apply.sum()), "max", int(n_apply.max()), "status", set(status.tolist()))
w, *_ = op.solve(w, tol=1e-10, algorithm="newton", inner_rtol=1e-12, inner_atol=0.0)
g = 0.5 + np.random.default_rng(1).random(shapes)
mom, n_iter, n_apply, rel, res_T, status, _ = op.adjoint(w, g, rtol=1e-10)
print("gradient: applications sum", int(n_apply.sum()), "max", int(n_apply.max()), "iterations sum", int(n_iter.sum()),
      "status", set(status.tolist()))
op.close()
