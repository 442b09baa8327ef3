"""
TEST INFRASTRUCTURE -- numpy restatement of the rule by which the continuous-state operator chooses, per grid
point, how it reads the iterate.  A restatement of this project's own code, formula by formula:

  host   sdfs_via_autodiff_amd/csrc/sdfs_api.hip   (sdfs_create_continuous, from its upload of the nodes to its end)
           cd.etamax   etamax[d] = max_m |eta[d][m]|
           tq          tensor-rule detection: M = tq^D (tq = 2 .. 64) and eta[d][m] = eta[d][((m / tq^d) % tq) tq^d]
           mext        mext[d] = the largest box extent any grid point asks for in dimension d, vmax = prod mext,
                       uomax = prod over all but the two fastest dimensions
           cd.cap      cap = min(vmax, 4000), rounded up to even
           cd.ucap     pre-contraction iff tq and vmax <= 4000 and uomax tq^2 + cap <= 4000; then ucap = uomax tq^2
           launch_cont dynamic LDS = 8 (cap + ucap) bytes for T, twice that for J.v
  kernel sdfs_via_autodiff_amd/csrc/cont_kernel.hpp
           :133-143    a[d], k[d]: the affine map node -> next-state coordinate of this block's grid point
           :152-164    blo / bext per dimension from the last dimension down; a block is staged while the running
                       product V bext[d] stays <= cap (once it fails it stays unstaged and V stops growing)
           :184-186    a staged block pre-contracts iff tq > 0 and (V / (bext[D-1] bext[D-2])) tq^2 <= ucap

The three paths a block can take:
  1  pre-contracted   staged and pre-contraction enabled
  2  staged           staged, full 2^D-corner fold from LDS (Monte Carlo, or a tensor rule whose U does not fit)
  3  global gather    not staged: corners from global memory through long long strides

Classes of a whole launch:  A every block on path 1,  B every block on path 2,  C staged and unstaged blocks mixed,
D no block staged.

The dynamics table (rho, xcoef / xdim, vol = sconst or phi exp(x[voldim])) restates the per-model branches of sdfs_create_continuous.
"""
import numpy as np

CAP_LIMIT = 4000            # sdfs_api.hip, sdfs_create_continuous: cap_limit


def dynamics(model, params):
    """Per dimension (rho, sconst, phi, voldim, xcoef, xdim); -1 = absent (sdfs_create_continuous, the model branches)."""
    q = [float(p) for p in params]
    if model == "ssy":          # dims h_lam, h_c, h_z, z
        return [(q[9], q[12], 0.0, -1, 0.0, -1), (q[8], q[11], 0.0, -1, 0.0, -1),
                (q[7], q[10], 0.0, -1, 0.0, -1), (q[4], 0.0, q[5], 2, 0.0, -1)]
    if model == "gcy":          # dims h_lam, h_c, h_z, h_zpi, z, z_pi
        return [(q[3], q[4], 0.0, -1, 0.0, -1), (q[10], q[11], 0.0, -1, 0.0, -1),
                (q[12], q[13], 0.0, -1, 0.0, -1), (q[16], q[17], 0.0, -1, 0.0, -1),
                (q[7], 0.0, q[9], 2, q[8], 5), (q[14], 0.0, q[15], 3, 0.0, -1)]
    raise ValueError(model)


def tensor_order(nodes):
    """tq of sdfs_create_continuous: the 1-D order of a tensor rule in gridmake order, else 0."""
    D, M = nodes.shape
    tq = next((c for c in range(2, 65) if c ** D == M), 0)
    if not tq:
        return 0
    m = np.arange(M)
    for d in range(D):
        st = tq ** d
        if np.any(nodes[d] != nodes[d][((m // st) % tq) * st]):
            return 0
    return tq


def box_extents(model, params, grids, nodes):
    """bext[d] of every grid point (cont_kernel.hpp:133-143, :152-160; the host evaluates the same expressions over
    (i, ix, iv) in sdfs_create_continuous's mext loop): a list of D integer arrays that broadcast against the grid's shape."""
    grids = [np.asarray(g, dtype=np.float64) for g in grids]
    nodes = np.asarray(nodes, dtype=np.float64)
    D = len(grids)
    n = [len(g) for g in grids]
    etamax = np.max(np.abs(nodes), axis=1)

    def axis(e):                # grid e as an array that broadcasts along dimension e of the full grid
        return grids[e].reshape([-1 if i == e else 1 for i in range(D)])

    out = []
    for d, (rho, sconst, phi, voldim, xcoef, xdim) in enumerate(dynamics(model, params)):
        lo, inv_step = grids[d][0], 1.0 / (grids[d][1] - grids[d][0])
        mean = rho * axis(d)
        if xdim >= 0:
            mean = mean + xcoef * axis(xdim)
        vol = phi * np.exp(axis(voldim)) if voldim >= 0 else np.float64(sconst)
        a = (mean - lo) * inv_step
        span = np.abs(vol * inv_step) * etamax[d]
        hi = float(n[d] - 1)
        cmin = np.minimum(np.maximum(a - span, 0.0), hi)
        cmax = np.minimum(np.maximum(a + span, 0.0), hi)
        blo = np.minimum(cmin.astype(np.int64), n[d] - 2)
        bhi = np.maximum(blo + 1, np.minimum(cmax.astype(np.int64) + 1, n[d] - 1))
        out.append(bhi - blo + 1)
    return out


def classify(model, params, grids, nodes):
    """The path rule for one operator.  nodes: (D, M) quadrature nodes or Monte-Carlo draws.  Returns a dict with
    mext (per dimension), vmax, uomax, cap, tq (0 = the host does not pre-contract), ucap, precontract, lds_T /
    lds_jvp (dynamic LDS bytes), staged (boolean array over the grid), n_staged, n_unstaged and cls in "ABCD"."""
    nodes = np.asarray(nodes, dtype=np.float64)
    D = len(grids)
    shape = tuple(len(g) for g in grids)
    bext = box_extents(model, params, grids, nodes)
    mext = [max(2, int(b.max())) for b in bext]
    vmax = int(np.prod(mext, dtype=np.int64))
    uomax = int(np.prod(mext[:D - 2], dtype=np.int64))
    cap = min(vmax, CAP_LIMIT)
    cap += cap & 1
    tq_rule = tensor_order(nodes)
    precontract = bool(tq_rule and vmax <= CAP_LIMIT and uomax * tq_rule * tq_rule + cap <= 4000)
    tq = tq_rule if precontract else 0
    ucap = uomax * tq * tq

    # cont_kernel.hpp:152-164, from the last dimension down
    staged = np.ones(shape, dtype=bool)
    V = np.ones(shape, dtype=np.int64)
    for d in range(D - 1, -1, -1):
        staged &= V * bext[d] <= cap
        V = np.where(staged, V * bext[d], V)
    # :184-186: with ucap = uomax tq^2 every staged block of a pre-contracting launch fits U
    if precontract:
        Vo = V // (bext[D - 1] * bext[D - 2])
        assert np.all(Vo[staged] * tq * tq <= ucap)

    ns = int(staged.sum())
    nu = staged.size - ns
    cls = "D" if ns == 0 else "C" if nu else "A" if precontract else "B"
    return dict(mext=mext, vmax=vmax, uomax=uomax, cap=cap, tq=tq, ucap=ucap, precontract=precontract,
                tq_rule=tq_rule, lds_T=8 * (cap + ucap), lds_jvp=16 * (cap + ucap), staged=staged,
                n_staged=ns, n_unstaged=nu, cls=cls)


# -- the case table of tests/test_hip_continuous_paths.py, pinned on the CPU by tests/test_cont_boxes_cpu.py ----------
# (name, model, sizes, num_std_devs, rule, class, staged blocks, unstaged blocks, cap or None)
# rule: ("gh", d) = Gauss-Hermite tensor rule of order d per dimension; ("mc", M) = M standard-normal draws from
# default_rng(1).standard_normal((D, M))
CASES = [
    ("A-ssy-headline", "ssy", (10, 10, 10, 20), 3.2, ("gh", 5), "A", 20000, 0, 856),
    ("A-gcy", "gcy", (3, 3, 3, 3, 8, 8), 1.0, ("gh", 4), "A", 5184, 0, 1216),
    ("B-ssy-refused", "ssy", (8, 8, 8, 16), 1.0, ("gh", 7), "B", 8192, 0, 3200),
    ("B-gcy-refused", "gcy", (4, 4, 4, 4, 6, 6), 0.5, ("gh", 3), "B", 9216, 0, 2880),
    ("B-ssy-mc", "ssy", (10, 10, 10, 20), 3.2, ("mc", 1000), "B", 20000, 0, None),
    ("C-ssy", "ssy", (12, 12, 12, 24), 1.0, ("gh", 5), "C", 6640, 34832, None),
    ("C-gcy", "gcy", (4, 5, 4, 5, 7, 6), 0.25, ("gh", 3), "C", 10144, 6656, None),
    ("C-gcy-almost-staged", "gcy", (4, 4, 4, 4, 6, 6), 0.3, ("gh", 3), "C", 9088, 128, None),
    ("C-gcy-mc", "gcy", (4, 4, 4, 4, 6, 6), 0.3, ("mc", 300), "C", 7424, 1792, None),
    ("D-ssy", "ssy", (9, 9, 9, 18), 0.4, ("gh", 5), "D", 0, 13122, None),
    ("D-gcy", "gcy", (4, 4, 4, 4, 6, 6), 0.1, ("gh", 3), "D", 0, 9216, None),
]
CASE_IDS = [c[0] for c in CASES]


def make_case(case):
    """(model, params, grids, nodes (D, M), weights or None) of one row of CASES, from the oracle's builders."""
    from oracle import continuous as OC
    from oracle import models as OM
    _, model, sizes, nsd, (kind, k) = case[:5]
    params = OM.ssy_params() if model == "ssy" else OM.gcy_params()
    grids = (OC.build_grid_ssy if model == "ssy" else OC.build_grid_gcy)(params, sizes, nsd)
    D = len(sizes)
    if kind == "gh":
        nodes, weights = OC.qnwnorm([k] * D)
        return model, params, grids, np.ascontiguousarray(nodes.T), weights
    return model, params, grids, np.random.default_rng(1).standard_normal((D, k)), None


def case_inputs(name):
    """The iterate w = 300 + 600 U(0, 1) and the direction v ~ N(0, 1) of one case (seeded by its row number)."""
    i = CASE_IDS.index(name)
    rng = np.random.default_rng(100 + i)
    shape = CASES[i][2]
    return 300.0 + 600.0 * rng.random(shape), rng.standard_normal(shape)


def oracle_task(name, what, k=1):
    """One oracle quantity of one case, rebuilt from the case's name alone so that it can run in a worker process
    (the oracle is a Python loop over grid points: seconds to tens of seconds per application at these sizes).
    what: "T" -> [T(w), T(T(w)), ...] (k applications), "jv" -> J(w) v, "jabs" -> J(w) |v|."""
    from oracle import continuous as OC
    model, params, grids, nodes, weights = make_case(CASES[CASE_IDS.index(name)])
    w, v = case_inputs(name)
    if what == "T":
        T = OC.T_fun_factory(model, params, grids, nodes, weights)
        out = []
        for _ in range(k):
            w = T(w)
            out.append(w)
        return out
    J = OC.jvp_factory(model, params, grids, nodes, weights)
    return J(w, v if what == "jv" else np.abs(v))
