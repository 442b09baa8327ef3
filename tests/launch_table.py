"""
The launch table: for the smallest shape on every path of the host layer, what one application launches (the text of
describe_plan(), the counter table of one T, one linearising T, one J.v, one (J - I).v and one J^T.u) and what it
computes (SHA-256 of every output), plus iteration counts and final errors of the three solver loops with the captured
graph and with plain launches.  tools/launch_table.py records it into tests/golden/launch_table.json,
tests/test_hip_launch_table.py recomputes it and requires equality.

Knobs are read when a handle is created, so every operator is built under its own environment.
"""
import contextlib
import hashlib
import os
import struct

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "launch_table.json")

# name -> (model, shapes, knobs)
GRID_CASES = {
    "generic ssy 2x3x4x5": ("ssy", (2, 3, 4, 5), dict(SDFS_PLAN="classic")),
    "generic gcy 2x3x2x3x2x3": ("gcy", (2, 3, 2, 3, 2, 3), dict(SDFS_PLAN="classic")),
    "small ssy 5x5x5x5": ("ssy", (5, 5, 5, 5), {}),
    "small gcy 3x3x3x3x3x3": ("gcy", (3, 3, 3, 3, 3, 3), {}),
    # (extents on both sides of 17 keep the generic tiles by default; SDFS_PAD_PLAN=2 puts the shape on the padded plan)
    "ssy 22x18x32x7": ("ssy", (22, 18, 32, 7), {}),
    "padded ssy 22x18x32x7": ("ssy", (22, 18, 32, 7), dict(SDFS_PAD_PLAN=2)),
    "pair ssy 16x16x16x16": ("ssy", (16, 16, 16, 16), dict(SDFS_PLAN="pair")),
    "pair ssy 16x16x16x16 unstreamed": ("ssy", (16, 16, 16, 16), dict(SDFS_PLAN="pair", SDFS_LINE_STREAM=0)),
}
STORAGE_CASE = "generic ssy 2x3x4x5"          # J.v under krylov_f32 = 1 and 2 through sdfs_debug_jvp_storage_dev
T32_CASE = "pair ssy 16x16x16x16"             # one T under opts.t_f32
CASES = list(GRID_CASES) + ["continuous ssy 3x4x3x5", "dense ssy 2x3x2x3"]

LOOP_CASES = {
    "small ssy 5x5x5x5": ("ssy", (5, 5, 5, 5), {}),
    "generic ssy 2x3x4x5": ("ssy", (2, 3, 4, 5), dict(SDFS_PLAN="classic")),
    "pair ssy 16x16x16x16": ("ssy", (16, 16, 16, 16), dict(SDFS_PLAN="pair")),
}
ALGORITHMS = ("successive_approx", "newton", "anderson")
LOOP_TOL, LOOP_MAX_ITER = 1e-6, 2000


@contextlib.contextmanager
def env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def build(S, model, shapes, **knobs):
    m = S.SSY() if model == "ssy" else S.GCY()
    arr = (S.discretize_ssy if model == "ssy" else S.discretize_gcy)(m, shapes)
    with env(**knobs):
        return S.KoopmansOperator(model, shapes, m.params, arr)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def counter_table(op):
    return [[c["name"], int(c["launches"]), float(c["alg_bytes"]), float(c["alg_flops"])] for c in op.counters()]


def inputs(shapes):
    rng = np.random.default_rng(11)
    return 400 + 500 * rng.random(shapes), rng.standard_normal(shapes)


def applications(op, vjp):
    """Counter table of T, linearising T, J.v, (J - I).v (and J^T.u) with profiling on; their hashes with it off."""
    import torch
    w, v = inputs(op.shapes)
    wd, vd = torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda()
    out = {k: torch.empty_like(wd) for k in ("T", "Tlin", "jvp", "jmi") + (("vjp",) if vjp else ())}
    torch.cuda.synchronize()

    def run():
        op.apply_dev(wd.data_ptr(), out["T"].data_ptr())
        op.linearize_dev(wd.data_ptr(), out["Tlin"].data_ptr())
        op.jvp_dev(vd.data_ptr(), out["jvp"].data_ptr())
        op.jvp_dev(vd.data_ptr(), out["jmi"].data_ptr(), minus_identity=True)
        if vjp:
            op.vjp_dev(vd.data_ptr(), out["vjp"].data_ptr())
        op.synchronize()

    op.set_profiling(True)
    op.reset_counters()
    run()
    table = counter_table(op)
    op.set_profiling(False)
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    run()
    return table, {k: sha(t.cpu().numpy()) for k, t in out.items()}


def storage_forms(S):
    """J.v on the generic tiles with fp32 Krylov storage (1) and its bf16-rounded form (2)."""
    import torch
    model, shapes, knobs = GRID_CASES[STORAGE_CASE]
    w, v = inputs(shapes)
    res = {}
    for mode in (1, 2):
        op = build(S, model, shapes, **knobs)
        wd, vd = torch.from_numpy(w).cuda(), torch.from_numpy(v.astype(np.float32)).cuda()
        out = torch.zeros_like(vd)
        torch.cuda.synchronize()
        op.set_profiling(True)
        op.reset_counters()
        op.debug_jvp_storage_dev(mode, wd.data_ptr(), vd.data_ptr(), out.data_ptr())
        op.synchronize()
        table = counter_table(op)
        op.set_profiling(False)
        out.zero_()
        torch.cuda.synchronize()
        op.debug_jvp_storage_dev(mode, wd.data_ptr(), vd.data_ptr(), out.data_ptr())
        op.synchronize()
        res["krylov_f32=%d" % mode] = dict(counters=table, hashes={"jvp": sha(out.cpu().numpy())})
    return res


def t32_form(S):
    """One T with fp32 intermediates (opts.t_f32) on the pair plan."""
    model, shapes, knobs = GRID_CASES[T32_CASE]
    op = build(S, model, shapes, **knobs)
    w, _ = inputs(shapes)
    op.set_profiling(True)
    op.reset_counters()
    op.solve(w, "successive_approx", tol=0.0, max_iter=1, t_f32=1)
    table = counter_table(op)
    op.set_profiling(False)
    x, _, _ = op.solve(w, "successive_approx", tol=0.0, max_iter=1, t_f32=1)
    return dict(counters=table, hashes={"T": sha(x)})


def special_operator(S, name):
    if name.startswith("continuous"):
        z = np.load(os.path.join(GOLD, "cont_ssy_3x4x3x5_sd1.0.npz"))
        grids = tuple(z[f"grid{i}"] for i in range(len(z["sizes"])))
        return S.T_fun_factory((z["params"], grids, z["nodes"], z["weights"]), "quadrature", z["w"].size)
    z = np.load(os.path.join(GOLD, "dense_ssy_2x3x2x3.npz"))
    p = tuple(z["params"])
    return S.DenseOperator(z["H"], float(p[0]), float((1 - p[1]) / (1 - 1 / p[2])))


def special_applications(op):
    """T and J.v (at a linearisation of its own) of the continuous or the dense operator."""
    import torch
    w, v = inputs(op.shapes)
    wd, vd = torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda()
    out = {k: torch.empty_like(wd) for k in ("T", "Tlin", "jvp")}
    torch.cuda.synchronize()

    def run():
        op.apply_dev(wd.data_ptr(), out["T"].data_ptr())
        op.linearize_dev(wd.data_ptr(), out["Tlin"].data_ptr())
        op.jvp_dev(vd.data_ptr(), out["jvp"].data_ptr())
        op.synchronize()

    op.set_profiling(True)
    op.reset_counters()
    run()
    table = counter_table(op)
    op.set_profiling(False)
    for t in out.values():
        t.zero_()
    torch.cuda.synchronize()
    run()
    return table, {k: sha(t.cpu().numpy()) for k, t in out.items()}


def record_case(S, name):
    if name in GRID_CASES:
        model, shapes, knobs = GRID_CASES[name]
        op = build(S, model, shapes, **knobs)
        table, hashes = applications(op, vjp=model == "ssy")      # (GCY's z tensor is conditional: no J^T.u)
    else:
        op = special_operator(S, name)
        table, hashes = special_applications(op)
    return dict(describe=op.describe_plan(), counters=table, hashes=hashes)


def record_loop(S, name, algorithm, use_graph):
    model, shapes, knobs = LOOP_CASES[name]
    op = build(S, model, shapes, **knobs)
    x, n, info = op.solve(np.full(shapes, 800.0), algorithm, tol=LOOP_TOL, max_iter=LOOP_MAX_ITER, use_graph=use_graph)
    return dict(n_iter=int(n), n_apply=int(info["n_apply"]), final_err=bits(info["final_err"]), status=int(info["status"]))


def loop_key(name, algorithm, use_graph):
    return "%s / %s / %s" % (name, algorithm, "graph" if use_graph else "launches")


def record_all(S):
    table = {name: record_case(S, name) for name in CASES}
    for k, v in storage_forms(S).items():
        table[STORAGE_CASE + " " + k] = v
    table[T32_CASE + " t_f32"] = t32_form(S)
    loops = {loop_key(n, a, g): record_loop(S, n, a, g) for n in LOOP_CASES for a in ALGORITHMS for g in (1, 0)}
    return dict(applications=table, loops=loops)
