"""
One batched solve for a counter run of its own (tools/README.md): SSY 10^4, B = 256, tol 1e-6.

    rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS \
        SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS --output-format csv -d OUT -- python tools/batch_pmc_run.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdfs_via_autodiff_amd as S                       # noqa: E402
from batch_family import member, package_model         # noqa: E402

models = [package_model(S, "ssy", member("ssy", b)) for b in range(256)]
res = S.solve_batch(models, (10,) * 4, tol=1e-6)
print("iterations", int(res.n_iter.min()), "...", int(res.n_iter.max()), "sum", int(res.n_iter.sum()), "status", set(res.status.tolist()))
