"""The problems, the extended-precision reference and the derived error bounds of
test_gpu_accuracy.py, which holds the Gram, solve and scoring kernels to the fp64 arithmetic
DESIGN section 3 promises, across conditioning.  Nothing here touches the GPU:
test_accuracy_cpu.py validates this yardstick (headroom of a plain fp64 numpy pipeline, what
each regime reaches, how many systems are asserted) where there is none.

Configurations (one per Gram / solve kernel pair):
  MF k = 8        k_gram_mf_stream, k_solve_tps, k_solve
  MF k = 16       k_gram_mf_stream, k_solve_quad and its coupled role
  MF k = 32, 64   k_gram_mf_mfma, k_solve_tile, k_solve
  NCF k = 8       k_ncf_gram_rows, k_solve_col
  NCF k = 16      k_ncf_gram_rows, k_ncf_query_pro + k_solve_rows
  NCF k = 32      k_ncf_gram_rows, k_solve_tile
  MF k = 128      k_big_gram, the k_bs_* panels with the narrow first panel, k_big_solve
  NCF k = 64      k_big_gram, k_bs_*, k_big_solve
MF k = 256 and NCF k = 128, 256 run the same large-k kernels at larger D and are left out for
time (their longdouble references alone take minutes).

Problem (one per configuration, Ds = k + 1 (MF), 2 k (NCF) the side block size): "ladder" items
with 1, 2, Ds - 1, Ds, Ds + 1, 2 Ds + 1 and 300 raters (rank-deficient, exactly full and
over-determined Grams; 300 crosses the 256-rating Gram slice of the k <= 16 and NCF passes) and
one list past the path's own Gram slice (4,100 at MF k = 32, 64: slices of 4,096; 2,049 at
large k: slices of 2,048); every other item has 3 raters; user 0 has 40 ratings; user U - 1 and
item I - 1 have none; one pair is in train twice; train rows permuted.

Regimes (embedding tables scaled in float32: the GPU and the reference see the same values):
  base       wd 1e-3, damping 1e-6
  nodecay    wd 0,    damping 1e-9
  small      embedding tables x 1e-3
  big        embedding tables x 30
  collinear  the raters of the (Ds + 1)-list and of the 300-list have user rows p0 + 1e-4 noise

Reference: theta, v, G, e, H restated from oracle/fia_oracle.py (_mf_core, _ncf_core,
ncf_forward_backward) at np.longdouble (80-bit, eps 1.1e-19) on the fp32 parameters widened
exactly, in the LIBRARY's block order (assemble_hessian): MF [p_u, b_u, q_i, b_i], NCF
[Pm_u, Pg_u, Qm_i, Qg_i].  The oracle's order is MF [p_u, q_i, b_u, b_i], NCF [Pm_u, Qm_i,
Pg_u, Qg_i]; lib_order() maps one to the other.

Backward error: eta(H, v, x) = |H x - v|_inf / (|H|_inf |x|_inf + |v|_inf), in longdouble.  An
uncoupled query's system is block diagonal and each side block is judged on its own (over the
whole vector an error in one block hides behind the other block's large x); a coupled query
(the pair is a train row; H indefinite) is judged on the full D system.

Bound per system (derived, not tuned):  eps64 (8 D rho + n_side g + c_G),  eps64 = 2^-53.
  * Solve.  Unpivoted LDL^T with fp64 FMA solves (H + dH) x = v with |dH| <= c D eps |L||D||L^T|
    (Higham, Accuracy and Stability, thm 10.4 with the two triangular solves: c < 4 for the
    factorisation and the substitutions together; 8 leaves room for the reciprocal-multiply
    the kernels use instead of a division and for assembling H from the Gram caches).
    rho = | |L||D||L^T| |_inf / |H|_inf is the growth of a plain numpy LDL^T in the library's
    order for a coupled system, and 2 flat for an SPD side block (there |L||D||L^T| <= D |H|
    in theory, 1.0 - 1.6 measured, and the side kernels eliminate in orders of their own).
  * Gram accumulation.  A sum of n_side products in fp64 is within gamma_n = n eps of exact
    relative to the sum of absolute values: |dH| <= n_side eps (2/n) |G|^T |G|, so
    g = | (2/n) |G|^T |G| |_inf / |H|_inf.
  * c_G.  MF: 0, the entries of G are fp32 parameters, exact in fp64, and so are their
    products.  NCF: a row of G is the fp64 MLP backward chain W1 (1[z1>0] (W2 (1[z2>0] W3m)))
    (k/2 then k FMAs per entry) or W3g * Qg (one rounding), so the computed row is within
    m eps g_abs of exact, m = 3k/2 + 2, g_abs the same chain on absolute values (masks kept).
    Then |dH| <= 2 m eps (2/n) G_abs^T G_abs and |dv| <= m eps v_abs, which in eta is at most
    c_G = 2 m | (2/n) G_abs^T G_abs |_inf / |H|_inf + m |v_abs|_inf / |v|_inf.
  A ReLU pre-activation within 1e-9 of 0 could flip between precisions; that is no kernel
  error, and reference() asserts that no row it uses has one.
No uncoupled system is judged by more than 1e-11 (UNCOUPLED_CAP): the derived bound is under
it everywhere (2.7e-12 at 4,100 ratings in `base`) except on the item block of the 4,100-list
at MF k = 64 in `big`, where the embedding columns outweigh the bias column, g = 22 and
4,100 g eps64 alone is 1.0e-11 (1.02e-11 - 1.06e-11 over five draws of the problem, so no
redraw helps).  There the system is held to the cap itself, the stricter of the two, and
CLAMPED records it; test_accuracy_cpu.py asserts that this is the only place.  A coupled system
is asserted against its bound only where rho <= 1e3 (RHO_CAP), which keeps the bound from being
vacuous.

Scoring bound (judged with the GPU's own x, apart from the solve's conditioning):
  infl_ld(x)_j = (2 e_j g_j + wd M theta) . x / n          per related rating j
  bound_j = eps64 4 (D + 2 k) S_j
  S_j = (2 |e_j| |g_j|.|x| + wd |M theta|.|x| + 2 E_j |g_j . x|) / n
  * the two dot products of D terms are within D eps of exact relative to their absolute sums
    (first two terms); e_j = r-hat_j - y_j is itself a sum of k + 4 terms (MF) or the forward
    pass (NCF, 2k + k + 3k/2 terms deep) computed in fp64, within (2 k) eps of exact relative
    to its absolute-valued evaluation E_j, and multiplies g_j . x (third term).  4 covers the
    final products, the division by n and FMA contraction orders.
  E_j: MF sum |p q| + |b_u| + |b_i| + |g| + |y|; NCF the forward pass on absolute values
  (|x0| |W1| + |b1|, then |W2|, |b2|, |W3|, |b3|) + |y|."""
import functools

import numpy as np

from influence import synth

LD = np.longdouble
EPS64 = 2.0 ** -53
UNCOUPLED_CAP = 1e-11
RHO_CAP = 1e3
RELU_MARGIN = 1e-9
CONFIGS = [("MF", 8), ("MF", 16), ("MF", 32), ("MF", 64), ("NCF", 8), ("NCF", 16), ("NCF", 32), ("MF", 128),
           ("NCF", 64)]
LARGE_K = [("MF", 128), ("NCF", 64)]
LONG_LIST = {("MF", 32): 4100, ("MF", 64): 4100, ("MF", 128): 2049, ("NCF", 64): 2049}   # past 4,096 / 2,048
SLICE_SMALL = 256                        # the Gram slice of the k <= 16 and NCF passes
REGIMES = {                              # wd, damping, embedding scale, collinear
    "base": (1e-3, 1e-6, 1.0, False),
    "nodecay": (0.0, 1e-9, 1.0, False),
    "small": (1e-3, 1e-6, 1e-3, False),
    "big": (1e-3, 1e-6, 30.0, False),
    "collinear": (1e-3, 1e-6, 1.0, True),
}
N_OTHER = 44                             # items of 3 raters; user 0 is a rater of the first 40
BIG_USER_DEG = 40
SEED = 90


def config_id(v):
    return "%s-%d" % v if isinstance(v, tuple) else None


def side_size(model, k):
    return k + 1 if model == "MF" else 2 * k


def lib_order(model, k):
    """x_lib = x_oracle[lib_order]: the library's block order from the oracle's."""
    a = np.arange(k)
    if model == "MF":
        return np.concatenate([a, [2 * k], k + a, [2 * k + 1]])
    return np.concatenate([a, 2 * k + a, k + a, 3 * k + a])


def ladder(model, k):
    Ds = side_size(model, k)
    out = [1, 2, Ds - 1, Ds, Ds + 1, 2 * Ds + 1, 300]
    if (model, k) in LONG_LIST:
        out.append(LONG_LIST[(model, k)])
    return out


# ---------------------------------------------------------------------------------------
# problems
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(model, k):
    """Returns U, I, train, qu, qi, kinds (per query: "rater", "short", "big", "empty_user",
    "empty_item", "twice", "none"), lengths (of ladder item j = 0 ..)."""
    rng = np.random.default_rng(SEED + k + (1000 if model == "NCF" else 0))
    lengths = ladder(model, k)
    nl = len(lengths)
    U = max(320, max(lengths) + 220)
    I = nl + N_OTHER + 1
    pool = np.arange(1, U - 1)
    us, its = [], []
    for j, n in enumerate(lengths):
        us.append(rng.choice(pool, n, replace=False))
        its.append(np.full(n, j))
    for m in range(N_OTHER):
        r = rng.choice(pool, 3, replace=False)
        if m < BIG_USER_DEG:
            r[0] = 0
        us.append(r)
        its.append(np.full(3, nl + m))
    twice_item = nl + N_OTHER - 2
    twice_user = int(us[-2][1])
    us.append(np.array([twice_user]))
    its.append(np.array([twice_item]))
    tu = np.concatenate(us).astype(np.int32)
    ti = np.concatenate(its).astype(np.int32)
    tr = rng.integers(1, 6, tu.size).astype(np.float32)
    both = np.nonzero((tu == twice_user) & (ti == twice_item))[0]
    tr[both[1]] = tr[both[0]] % 5 + 1
    perm = rng.permutation(tu.size)
    tu, ti, tr = tu[perm], ti[perm], tr[perm]
    deg_u = np.bincount(tu, minlength=U)
    qs = []
    for j, n in enumerate(lengths):
        lst = tu[ti == j]                          # item j's list in index (train-row) order
        short = np.setdiff1d(np.nonzero((deg_u > 0) & (deg_u <= 8))[0], np.append(lst, 0))
        qs += [(int(lst[n // 2]), j, "rater"), (int(rng.choice(short)), j, "short"), (0, j, "big"),
               (U - 1, j, "empty_user")]
    qs += [(0, I - 1, "empty_item"), (twice_user, twice_item, "twice")]
    qs.insert(len(qs) // 2, (U - 1, I - 1, "none"))        # n = 0, in the middle of the batch
    qu = np.array([q[0] for q in qs], np.int32)
    qi = np.array([q[1] for q in qs], np.int32)
    return U, I, (tu, ti, tr), qu, qi, [q[2] for q in qs], lengths


def assert_problem_claims(model, k):
    U, I, train, qu, qi, kinds, lengths = problem(model, k)
    tu, ti, tr = train
    deg_u, deg_i = np.bincount(tu, minlength=U), np.bincount(ti, minlength=I)
    nl = len(lengths)
    assert list(deg_i[:nl]) == lengths and deg_i[I - 1] == 0 and deg_u[U - 1] == 0
    assert deg_u[0] == BIG_USER_DEG and not np.isin(ti[tu == 0], np.arange(nl)).any()
    assert set(deg_i[nl:I - 1]) == {3, 4} and (deg_i[nl:I - 1] == 4).sum() == 1
    assert 300 > SLICE_SMALL and (np.diff(ti) < 0).any() and (np.diff(tu) < 0).any()
    key = tu.astype(np.int64) * I + ti
    in_train = np.isin(qu.astype(np.int64) * I + qi, key)
    want = [kd in ("rater", "twice") for kd in kinds]
    assert list(in_train) == want
    t = kinds.index("twice")
    rows = np.nonzero((tu == qu[t]) & (ti == qi[t]))[0]
    assert rows.size == 2 and tr[rows[0]] != tr[rows[1]] and np.unique(key).size == key.size - 1
    n = deg_u[qu] + deg_i[qi]
    assert list(n == 0) == [kd == "none" for kd in kinds] and 30 <= qu.size <= 44
    return U, I, train, qu, qi, kinds, lengths


@functools.lru_cache(maxsize=None)
def params_for(model, k, regime):
    """fp32 parameters of a regime, in the order of synth's dicts."""
    U, I, train, _, _, _, lengths = problem(model, k)
    wd, damping, scale, collinear = REGIMES[regime]
    p = dict(synth.mf_params(U, I, k, SEED) if model == "MF" else synth.ncf_params(U, I, k, SEED))
    emb = [n for n in p if "/embedding_" in n]
    assert len(emb) == (2 if model == "MF" else 4)
    for n in emb:
        p[n] = (p[n] * np.float32(scale)).astype(np.float32)
    if collinear:
        tu, ti, _ = train
        Ds = side_size(model, k)
        raters = np.unique(tu[np.isin(ti, [lengths.index(Ds + 1), lengths.index(300)])])
        rng = np.random.default_rng(SEED + 1)
        for n in emb:
            if "users" in n:
                t = p[n].reshape(U, k).copy()
                t[raters] = (t[raters[0]][None, :] + np.float32(1e-4)
                             * rng.standard_normal((raters.size, k)).astype(np.float32)).astype(np.float32)
                p[n] = t.reshape(-1)
    return p


# ---------------------------------------------------------------------------------------
# the model at a given precision (restated from oracle/fia_oracle.py)
# ---------------------------------------------------------------------------------------
def tables(model, params, k, dt):
    f = lambda name: np.asarray(params[name], np.float32).astype(dt)
    if model == "MF":
        return dict(P=f("embedding_layer/embedding_users").reshape(-1, k),
                    Q=f("embedding_layer/embedding_items").reshape(-1, k),
                    bu=f("embedding_layer/bias_users"), bi=f("embedding_layer/bias_items"),
                    g=f("embedding_layer/global_bias")[0])
    h = k // 2
    return dict(Pm=f("embedding_layer/mlp/embedding_users").reshape(-1, k),
                Qm=f("embedding_layer/mlp/embedding_items").reshape(-1, k),
                Pg=f("embedding_layer/gmf/embedding_users").reshape(-1, k),
                Qg=f("embedding_layer/gmf/embedding_items").reshape(-1, k),
                W1=f("h1/weights").reshape(2 * k, k), b1=f("h1/biases"), W2=f("h2/weights").reshape(k, h),
                b2=f("h2/biases"), W3=f("h3/weights"), b3=f("h3/biases")[0])


def rows_of(model, T, k, users, items):
    """For rows (a, b): r-hat, its absolute-valued evaluation, the user-side and item-side
    blocks of d r-hat / d theta in library order ([q_b, 1] / [p_a, 1]; [dPm, dPg] / [dQm, dQg]),
    their absolute-valued chains, and the smallest |ReLU pre-activation|."""
    users = np.asarray(users, np.int64)
    items = np.asarray(items, np.int64)
    dt = T["P" if model == "MF" else "Pm"].dtype
    one = np.ones((users.size, 1), dt)
    if model == "MF":
        p, q = T["P"][users], T["Q"][items]
        r = (p * q).sum(1) + T["bu"][users] + T["bi"][items] + T["g"]
        ra = (np.abs(p * q)).sum(1) + np.abs(T["bu"][users]) + np.abs(T["bi"][items]) + np.abs(T["g"])
        gu, gi = np.concatenate([q, one], 1), np.concatenate([p, one], 1)
        return r, ra, gu, gi, np.abs(gu), np.abs(gi), np.inf
    h = k // 2
    W1, W2, W3m, W3g = T["W1"], T["W2"], T["W3"][:h], T["W3"][h:]
    x0 = np.concatenate([T["Pm"][users], T["Qm"][items]], 1)
    z1 = x0 @ W1 + T["b1"]
    h1 = np.maximum(z1, 0)
    z2 = h1 @ W2 + T["b2"]
    h2 = np.maximum(z2, 0)
    pg, qg = T["Pg"][users], T["Qg"][items]
    r = h2 @ W3m + (pg * qg) @ W3g + T["b3"]
    ra = ((np.abs(x0) @ np.abs(W1) + np.abs(T["b1"])) @ np.abs(W2) + np.abs(T["b2"])) @ np.abs(W3m) \
        + np.abs(pg * qg) @ np.abs(W3g) + np.abs(T["b3"])
    m1, m2 = z1 > 0, z2 > 0
    dx0 = (((W3m[None, :] * m2) @ W2.T) * m1) @ W1.T
    dx0a = (((np.abs(W3m)[None, :] * m2) @ np.abs(W2).T) * m1) @ np.abs(W1).T
    gu = np.concatenate([dx0[:, :k], W3g[None, :] * qg], 1)
    gi = np.concatenate([dx0[:, k:], W3g[None, :] * pg], 1)
    gua = np.concatenate([dx0a[:, :k], np.abs(W3g[None, :] * qg)], 1)
    gia = np.concatenate([dx0a[:, k:], np.abs(W3g[None, :] * pg)], 1)
    margin = min(np.abs(z1).min(initial=np.inf), np.abs(z2).min(initial=np.inf))
    return r, ra, gu, gi, gua, gia, float(margin)


def decay_mask(model, k):
    """M over one side block: MF biases are not decayed, every NCF table is."""
    Ds = side_size(model, k)
    m = np.ones(Ds)
    if model == "MF":
        m[k] = 0.0
    return m


def side_theta(model, T, k, sd, e):
    if model == "MF":
        return np.append(T["PQ"[sd]][e], T[("bu", "bi")[sd]][e])
    return np.concatenate([T[("Pm", "Qm")[sd]][e], T[("Pg", "Qg")[sd]][e]])


def seq_gram(G):
    """sum_j g_j g_j^T accumulated in list order at G's precision."""
    A = np.zeros((G.shape[1], G.shape[1]), G.dtype)
    for g in G:
        A += np.outer(g, g)
    return A


class Entity(object):
    """One side's list of one entity: rows (index order), per row e, E (absolute-valued
    residual), g (this side's block), g_abs, and the Grams sum g g^T, sum |g||g|^T,
    sum g_abs g_abs^T."""

    def __init__(self, model, T, k, train, sd, ent, rows, sequential):
        tu, ti, tr = train
        self.rows = rows
        r, ra, gu, gi, gua, gia, self.margin = rows_of(model, T, k, tu[rows], ti[rows])
        y = tr[rows].astype(r.dtype)
        self.e, self.E = r - y, ra + np.abs(y)
        self.g, self.gabs = (gu, gua) if sd == 0 else (gi, gia)
        self.other = (gi, gu)[sd]                  # the other side's block of the same rows
        self.other_ids = (ti, tu)[sd][rows]
        if sequential:
            self.A = seq_gram(self.g)
        else:
            self.A = self.g.T @ self.g
            self.Aabs = np.abs(self.g).T @ np.abs(self.g)
            self.Agabs = self.gabs.T @ self.gabs


class Reference(object):
    """The systems of a (configuration, regime) at precision dt (np.longdouble: the reference;
    np.float64 with sequential Grams: the plain fp64 pipeline of test_accuracy_cpu.py)."""

    def __init__(self, model, k, regime, dt=LD):
        assert dt is not LD or np.finfo(LD).eps < 1e-18, "np.longdouble is not extended precision here"
        self.model, self.k, self.regime, self.dt = model, k, regime, dt
        self.U, self.I, self.train, self.qu, self.qi, self.kinds, self.lengths = problem(model, k)
        self.wd, self.damping = REGIMES[regime][:2]
        self.params = params_for(model, k, regime)
        self.T = tables(model, self.params, k, dt)
        self.Ds = side_size(model, k)
        self.D = 2 * self.Ds
        tu, ti, _ = self.train
        self.lists = []
        for ids, n in ((tu, self.U), (ti, self.I)):
            order = np.argsort(ids, kind="stable").astype(np.int64)
            self.lists.append((order, np.searchsorted(ids[order], np.arange(n + 1), side="left")))
        self._ent = {}
        self._sys = {}

    def entity(self, sd, e):
        if (sd, e) not in self._ent:
            order, ptr = self.lists[sd]
            ent = Entity(self.model, self.T, self.k, self.train, sd, e, order[ptr[e]:ptr[e + 1]],
                         sequential=self.dt is not LD)
            assert ent.margin >= RELU_MARGIN, ("a ReLU pre-activation near 0: redraw", sd, e, ent.margin)
            self._ent[(sd, e)] = ent
        return self._ent[(sd, e)]

    def related(self, u, i):
        return np.concatenate([self.entity(0, u).rows, self.entity(1, i).rows])

    def system(self, q):
        """dict(n, coupled, H, Habs, Hgabs, v, vabs, theta, Mtheta) of query q in library order
        (Habs = (2/n) |G|^T |G|, Hgabs the same with g_abs)."""
        if q in self._sys:
            return self._sys[q]
        u, i = int(self.qu[q]), int(self.qi[q])
        return self._sys.setdefault(q, self.system_of(u, i))

    def system_of(self, u, i):
        model, k, Ds, D, dt = self.model, self.k, self.Ds, self.D, self.dt
        eu, ei = self.entity(0, u), self.entity(1, i)
        n = eu.rows.size + ei.rows.size
        r, _, gu, gi, gua, gia, margin = rows_of(model, self.T, k, [u], [i])
        assert margin >= RELU_MARGIN, ("a ReLU pre-activation near 0: redraw", u, i, margin)
        v, vabs = np.concatenate([gu[0], gi[0]]), np.concatenate([gua[0], gia[0]])
        theta = np.concatenate([side_theta(model, self.T, k, 0, u), side_theta(model, self.T, k, 1, i)])
        M = np.tile(decay_mask(model, k), 2).astype(dt)
        out = dict(n=n, v=v, vabs=vabs, theta=theta, Mtheta=M * theta, u=u, i=i)
        if n == 0:
            return out
        own = eu.other_ids == i                    # the pair's rows, in the user's list
        cdup = int(own.sum())
        s2n = dt(2) / dt(n)
        mats = []
        for name in ("A", "Aabs", "Agabs"):
            if not hasattr(eu, name):
                mats.append(None)
                continue
            H = np.zeros((D, D), dt)
            H[:Ds, :Ds], H[Ds:, Ds:] = getattr(eu, name), getattr(ei, name)
            if cdup:                               # each copy is in rel twice, with both blocks
                w = {"A": v, "Aabs": np.abs(v), "Agabs": vabs}[name]
                H += cdup * np.outer(w, w)
                H[:Ds, Ds:] += cdup * np.outer(w[:Ds], w[Ds:])
                H[Ds:, :Ds] += cdup * np.outer(w[Ds:], w[:Ds])
            mats.append(s2n * H)
        H, Habs, Hgabs = mats
        if cdup:
            s = s2n * 2 * eu.e[own].sum()
            a = np.arange(k)
            if model == "MF":                      # d2 r / dp_u dq_i = I
                H[a, Ds + a] += s
                H[Ds + a, a] += s
            else:                                  # d2 r / dPg_u dQg_i = diag(W3g)
                W3g = self.T["W3"][k // 2:]
                H[k + a, Ds + k + a] += s * W3g
                H[Ds + k + a, k + a] += s * W3g
        H[np.arange(D), np.arange(D)] += dt(self.wd) * M + dt(self.damping)
        out.update(coupled=cdup > 0, H=H, Habs=Habs, Hgabs=Hgabs, n_side=(eu.rows.size, ei.rows.size))
        return out

    # -------------------------------------------------------------------------------
    def influence(self, q, x):
        """infl_ld(x) and the scoring bound per related rating of query q, x in library order."""
        s = self.system(q)
        eu, ei = self.entity(0, s["u"]), self.entity(1, s["i"])
        Ds, dt, n = self.Ds, self.dt, s["n"]
        x = np.asarray(x, np.float64).astype(dt)
        gx, gax, e, E = [], [], [], []
        for sd, ent in ((0, eu), (1, ei)):
            mine, other = x[sd * Ds:(sd + 1) * Ds], x[(1 - sd) * Ds:(2 - sd) * Ds]
            own = ent.other_ids == (s["i"], s["u"])[sd]
            gx.append(ent.g @ mine + own * (ent.other @ other))
            gax.append(np.abs(ent.g) @ np.abs(mine) + own * (np.abs(ent.other) @ np.abs(other)))
            e.append(ent.e)
            E.append(ent.E)
        gx, gax, e, E = (np.concatenate(a) for a in (gx, gax, e, E))
        wd = dt(self.wd)
        infl = (2 * e * gx + wd * (s["Mtheta"] @ x)) / n
        S = (2 * np.abs(e) * gax + wd * (np.abs(s["Mtheta"]) @ np.abs(x)) + 2 * E * np.abs(gx)) / n
        return infl, EPS64 * 4 * (self.D + 2 * self.k) * S


# ---------------------------------------------------------------------------------------
# backward error, growth, bounds
# ---------------------------------------------------------------------------------------
def norm_inf(A):
    A = np.abs(A)
    return A.sum(1).max() if A.ndim == 2 else A.max()


def eta(H, v, x):
    x = np.asarray(x).astype(LD)
    H, v = np.asarray(H).astype(LD), np.asarray(v).astype(LD)
    return float(norm_inf(H @ x - v) / (norm_inf(H) * norm_inf(x) + norm_inf(v)))


def ldlt(H):
    """Unpivoted LDL^T at H's precision: unit lower L, d."""
    n = H.shape[0]
    L, d = np.eye(n, dtype=H.dtype), np.zeros(n, H.dtype)
    for j in range(n):
        w = L[j, :j] * d[:j]
        d[j] = H[j, j] - L[j, :j] @ w
        L[j + 1:, j] = (H[j + 1:, j] - L[j + 1:, :j] @ w) / d[j]
    return L, d


def ldlt_solve(H, v):
    L, d = ldlt(H)
    n = v.size
    y = v.copy()
    for j in range(n):
        y[j + 1:] -= L[j + 1:, j] * y[j]
    y /= d
    for j in range(n - 1, -1, -1):
        y[:j] -= L[j, :j] * y[j]
    return y


def growth(H):
    """rho = | |L||D||L^T| |_inf / |H|_inf of the fp64 unpivoted LDL^T of H (library order)."""
    H64 = np.asarray(H).astype(np.float64)
    L, d = ldlt(H64)
    L = np.abs(L)
    return float(norm_inf((L * np.abs(d)[None, :]) @ L.T) / norm_inf(H64))


CLAMPED = {}                             # (model, k, regime, query, side) -> the derived bound above the cap


def systems(ref, q):
    """The systems query q is judged by: [(name, index slice, H, v, bound or None, rho)].  An
    uncoupled query gives its two side blocks (rho = 2 flat), a coupled one the full system
    (bound None above RHO_CAP)."""
    s = ref.system(q)
    if s["n"] == 0:
        return []
    k, Ds, D = ref.k, ref.Ds, ref.D
    m = 3 * k // 2 + 2 if ref.model == "NCF" else 0

    def bound(sl, dim, rho, n_side):
        H = s["H"][sl, sl]
        hn = norm_inf(H)
        g = norm_inf(s["Habs"][sl, sl]) / hn
        cG = 0.0
        if m:
            cG = 2 * m * norm_inf(s["Hgabs"][sl, sl]) / hn + m * norm_inf(s["vabs"][sl]) / norm_inf(s["v"][sl])
        return float(EPS64 * (8 * dim * rho + n_side * g + cG))

    if s["coupled"]:
        sl = slice(0, D)
        rho = growth(s["H"])
        b = bound(sl, D, rho, s["n"]) if rho <= RHO_CAP else None
        return [("coupled", sl, s["H"], s["v"], b, rho)]
    out = []
    for sd, name in enumerate(("user", "item")):
        sl = slice(sd * Ds, (sd + 1) * Ds)
        b = bound(sl, Ds, 2.0, s["n_side"][sd])
        if b > UNCOUPLED_CAP:                      # held to the cap instead: never a wider check
            CLAMPED[(ref.model, k, ref.regime, q, name)] = b
            b = UNCOUPLED_CAP
        out.append((name, sl, s["H"][sl, sl], s["v"][sl], b, 2.0))
    return out


@functools.lru_cache(maxsize=None)
def reference(model, k, regime):
    """The longdouble reference of a (configuration, regime), computed once and shared
    (read-only)."""
    return Reference(model, k, regime, LD)


def judge(ref, x_of):
    """Records (query, system name, eta of x_of(q)[slice], bound or None, rho) of every system
    of ref's queries; x_of(q) is the query's x in library order."""
    out = []
    for q in range(ref.qu.size):
        for name, sl, H, v, b, rho in systems(ref, q):
            out.append((q, name, eta(H, v, np.asarray(x_of(q))[sl]), b, rho))
    return out


def summary(records):
    """Largest eta and bound of the asserted side blocks / coupled systems, the largest rho, and
    the largest eta above the cap: the rows of profiles/accuracy.md."""
    side = [r for r in records if r[1] != "coupled"]
    cpl = [r for r in records if r[1] == "coupled" and r[3] is not None]
    over = [r for r in records if r[1] == "coupled" and r[3] is None]
    mx = lambda rs, j: max([r[j] for r in rs], default=0.0)
    return dict(side_eta=mx(side, 2), side_bound=mx(side, 3), side_ratio=max([r[2] / r[3] for r in side], default=0.0),
                coupled_eta=mx(cpl, 2), coupled_bound=mx(cpl, 3),
                coupled_ratio=max([r[2] / r[3] for r in cpl], default=0.0), coupled_asserted=len(cpl),
                rho_max=mx(cpl + over, 4), over_cap=len(over), over_cap_eta=mx(over, 2))
