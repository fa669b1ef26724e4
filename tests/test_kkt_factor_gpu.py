"""KKT formation, factor and inverse on every route behind pq_factor_batched, and pq_factor_large:

    K = ps P + pd I + sigma I + Cg' R Cg + R_box     (form_elem / rho_for, chol_dev.h)

with per-problem rho, against tests/admm_reference.py::kkt_matrix in np.longdouble formed from
the same host arrays (ps P + pd I in longdouble too).  Every case asserts its route first
(pq_factor_last_route: 0 k_factor, 1 k_factor_sk, 2 k_factor_res), steered by the batch size
and the form alone (PQ_FACTOR_SK / PQ_FACTOR_RES are not set).

Forms (FORMS): p_scale / p_diag present and absent, sigma 0 and 1e-6, mg 0 / 1 / 4 / 64 with
rows of every kind (equality, one-sided, two-sided, both bounds infinite: general_rows), no box
and the mixed box (ordinary, fixed, free and one-sided variables: mixed_box), constraints
shared (strides 0) and per problem.  ws.rho is overwritten with values 0.02 .. 2 over the 8
distinct problems a batch cycles through; batch B takes problem b % 8.

Shapes: n = 24 (one 64-block, nvalid 24: a partly valid 16-block inside tile_chol_inv64), 64
(exactly one block), 65 (a second block with one valid row and column), 130 (ld 192, three
block columns: gemm_sk splits 4 and 8 chunks between its teams, 12 at the trtri step), 300 (ld
320, beyond PQ_RES_NMAX = 288, five block columns).

Bars, all computed in longdouble on the host for the problems with info == 0:
  factor   max|L L' - K| <= 8 r_np + eps max|K|,  r_np the same residual of
           numpy.linalg.cholesky of K rounded to float64 (a backward-error bar: it does not
           move with cond(K), which eq_scale puts at 1e5 .. 1e7 here)
  inverse  max|K Kinv - I| <= 8 r_np + 1e-15,  r_np the same residual of numpy.linalg.inv;
           invert = 2: Kinv == Kinv' exactly; invert = 1: the lower triangle alone is read
  padding  rows and columns >= n hold the identity
  routes   0 and 1 on the same input: max|K0 - K1| <= 10 max|K1 - Kinv_ld| (summation order)
8 is the margin of test_factor_resident_gpu.py::test_capacitance_like_ill_conditioned for a
kernel-versus-LAPACK residual, 10 the project's margin between summation orders.  In a batch
that cycles, the repeats of a problem are compared with its first occurrence (equal bit for
bit: the same kernel on the same input), which is compared with the reference.

Non-PD contract (test_non_pd_*): info is nonzero iff K is not PD and names the 16-column block
of the first failing pivot c: info == 1 + 16 (c // 16), status PQ_NON_CONVEX -- on the three
routes and pq_factor_large alike, for a negative pivot and for a NaN.

Measured on an MI355X (256 CUs: the large batches are 257 problems), worst over each batch of
8 x residual / bar, i.e. the kernel's residual in units of LAPACK's (the bar is at 8):
  route 0 factor    0.8 .. 3.7, and 6.6 at n = 24 mg4-box-shared (n = 300: 2.1, 3.6)
  route 0 inverse   1.6 .. 3.1 (n = 300, 257 problems: 2.2)
  route 1 inverse   1.5 .. 3.0          route 2, scaled form   2.5 (n = 65), 3.6 (n = 284)
  pq_factor_large   0.7 .. 3.7 (factor), 1.3 .. 3.1 (inverse)
  routes 0 and 1    |K0 - K1| 0 .. 5.3e-15 against |K1 - Kinv_ld| 7.7e-16 .. 2.5e-14 (at most 1.3 x)
No case misses a bar; every non-PD report equals 1 + 16 (c // 16) on all four entries.
"""
import ctypes

import numpy as np
import pytest
import torch

from porqua_amd import _lib, engine
from tests.admm_reference import LD, kkt_matrix, ref_settings
from tests.dense_cases import general_rows, mixed_box

pytestmark = pytest.mark.gpu

ROUTE_GEN, ROUTE_SK, ROUTE_RES, LARGE = 0, 1, 2, "large"
D = 8   # distinct problems a batch cycles through

# name: (p_scale / p_diag, sigma, mg, box, per-problem constraints)
FORMS = {
    "plain": (False, 0.0, 0, False, False),
    "scaled": (True, 1e-6, 0, False, False),
    "mg1-shared": (True, 0.0, 1, False, False),
    "mg4-box-shared": (False, 1e-6, 4, True, False),
    "mg4-box-per": (True, 1e-6, 4, True, True),
    "box-per": (True, 0.0, 0, True, True),
    "mg64-per": (True, 0.0, 64, False, True),
    "mg64-box-shared": (False, 1e-6, 64, True, False),
}
CONSTRAINED = [f for f, v in FORMS.items() if v[2] or v[3]]


def _cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


_hosts = {}


def _host(n, form):
    """The D distinct problems of (n, form) on the host, and their longdouble K (cached)."""
    key = (n, form)
    if key not in _hosts:
        scaled, sigma, mg, box, per = FORMS[form]
        rng = np.random.default_rng(1000 * n + sorted(FORMS).index(form))
        M = rng.standard_normal((D, n + 7, n))
        P = np.einsum("bki,bkj->bij", M, M) / n + 0.1 * np.eye(n)
        nc = D if per else 1
        h = dict(n=n, form=form, P=P, sigma=sigma, mg=mg, nc=nc,
                 ps=rng.uniform(0.5, 2.0, D) if scaled else None, pd=rng.uniform(0.01, 0.1, D) if scaled else None,
                 rho=np.geomspace(0.02, 2.0, D), rows=general_rows(n, mg, nc, 7 * n + mg) if mg else None,
                 box=mixed_box(n, nc) if box else None, K={}, refs={})
        _hosts[key] = h
    return _hosts[key]


def _K_ref(h, d, P=None):
    """kkt_matrix of distinct problem d in longdouble (``P``: a changed copy of its P)."""
    if P is None and d in h["K"]:
        return h["K"][d]
    n, c = h["n"], d % h["nc"]
    Pl = (h["P"][d] if P is None else P).astype(LD)
    if h["ps"] is not None:
        Pl = LD(h["ps"][d]) * Pl
        Pl[np.diag_indices(n)] += LD(h["pd"][d])
    Cg, lg, ug = (a[c] for a in h["rows"]) if h["mg"] else (np.zeros((0, n)), [], [])
    lb, ub = (a[c] for a in h["box"]) if h["box"] else (None, None)
    K = kkt_matrix(Pl, Cg, lg, ug, lb, ub, h["rho"][d], ref_settings(sigma=h["sigma"]), LD)
    if P is None:
        h["K"][d] = K
    return K


def _run(device, h, B, invert, route, idx=None, P=None):
    """pq_init_state, ws.rho overwritten per problem, ws.K pre-filled with NaN, then pq_factor_batched
    (or pq_factor_large: route LARGE) on problems b % D of the host set ``h`` (``P``: a (D, n, n) stack
    in place of its own).  Asserts the route; returns K (B, ld, ld), Dt, info, status."""
    lib = _lib.load()
    n, mg, nc = h["n"], h["mg"], h["nc"]
    cyc = np.arange(B) % D
    per = nc > 1
    qb = engine.QPBatch(n, B, mg, device=device, shared_constraints=not per, has_box=h["box"] is not None,
                        P=torch.empty(0, dtype=torch.float64, device=device))
    ld = qb.ld
    Pp = np.zeros((D, ld, ld))
    Pp[:, :n, :n] = h["P"] if P is None else P
    sel = torch.from_numpy(cyc).to(device)
    qb.P = torch.from_numpy(Pp).to(device)[sel].contiguous()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if h["ps"] is not None:
        qb.p_scale, qb.p_diag = dev(h["ps"][cyc]), dev(h["pd"][cyc])
    pick = cyc if per else np.zeros(1, dtype=int)
    if mg:
        Cg, lg, ug = h["rows"]
        Cp = np.zeros((nc, mg, ld))
        Cp[:, :, :n] = Cg
        qb.Cg, qb.lg, qb.ug = dev(Cp[pick]), dev(lg[pick]), dev(ug[pick])
    if h["box"] is not None:
        lo, up = np.full((nc, ld), -np.inf), np.full((nc, ld), np.inf)
        lo[:, :n], up[:, :n] = h["box"]
        qb.lb, qb.ub = dev(lo[pick]), dev(up[pick])
    s = engine.Settings(sigma=h["sigma"]).to_c()
    ws = engine.Workspace(qb)
    pb, st, strm = qb.c_struct(), ws.c_struct(), engine._stream()
    _lib.check(lib.pq_init_state(ctypes.byref(pb), ctypes.byref(st), None, 0, ctypes.byref(s), strm), "init")
    ws.rho.copy_(dev(h["rho"][cyc]))
    ws.K.fill_(float("nan"))
    ws.Dt.fill_(float("nan"))
    if idx is None:
        ip, ni = None, 0
    else:
        it = torch.tensor(idx, dtype=torch.int32, device=device)
        ip, ni = engine._ptr(it), len(idx)
    if route == LARGE:
        W = torch.empty((max(ni, 1) if idx is not None else B, ld, ld), dtype=torch.float64, device=device)
        _lib.check(lib.pq_factor_large(ctypes.byref(pb), ctypes.byref(st), ip, ni, ctypes.byref(s), invert,
                                       W.data_ptr(), W.stride(0), strm), "pq_factor_large")
    else:
        _lib.check(lib.pq_factor_batched(ctypes.byref(pb), ctypes.byref(st), ip, ni, ctypes.byref(s), invert, strm),
                   "pq_factor_batched")
        assert int(lib.pq_factor_last_route()) == route, (int(lib.pq_factor_last_route()), route)
    torch.cuda.synchronize()
    return ws.K.cpu().numpy(), ws.Dt.cpu().numpy(), ws.info.cpu().numpy(), ws.status.cpu().numpy()


# ---- the bars ------------------------------------------------------------------------------------

def _amax(a):
    return float(np.abs(a).max())


def _bars(h, d):
    """(factor bar, inverse bar) of distinct problem d from LAPACK's residuals in longdouble (cached)."""
    if d not in h["refs"]:
        Kl = _K_ref(h, d)
        K64 = np.asarray(Kl, dtype=np.float64)
        L = np.linalg.cholesky(K64).astype(LD)
        r_chol = _amax(L @ L.T - Kl)
        r_inv = _amax(Kl @ np.linalg.inv(K64).astype(LD) - np.eye(h["n"], dtype=LD))
        h["refs"][d] = (8.0 * r_chol + float(np.finfo(np.float64).eps) * _amax(Kl), 8.0 * r_inv + 1e-15)
    return h["refs"][d]


def _inverse_ld(h, d):
    """K^-1 of distinct problem d in longdouble: LAPACK's, then three Newton steps on longdouble residuals."""
    Kl = _K_ref(h, d)
    I = np.eye(h["n"], dtype=LD)
    X = np.linalg.inv(np.asarray(Kl, dtype=np.float64)).astype(LD)
    for _ in range(3):
        X = X + X @ (I - Kl @ X)
    assert _amax(Kl @ X - I) <= 1e-16
    return X


def _check_padding(Kb, n, invert):
    ld = Kb.shape[0]
    low = np.tril(Kb)
    assert np.array_equal(low[n:, n:], np.eye(ld - n)) and not low[n:, :n].any()
    if invert == 2:
        assert np.array_equal(Kb[n:, n:], np.eye(ld - n)) and not Kb[:n, n:].any()


def _check_problem(tag, h, d, Kb, invert, worst):
    """One factored (invert 0) or inverted problem against the bars; worst collects 8 x residual / bar."""
    n = h["n"]
    Kl = _K_ref(h, d)
    bar_f, bar_i = _bars(h, d)
    assert np.isfinite(np.tril(Kb)).all(), tag
    _check_padding(Kb, n, invert)
    if invert == 0:
        L = np.tril(Kb[:n, :n]).astype(LD)
        r, bar = _amax(L @ L.T - Kl), bar_f
        assert not np.triu(Kb[:n, :n], 1)[np.arange(n)[:, None] // 64 == np.arange(n)[None, :] // 64].any()
    else:
        A = Kb[:n, :n]
        if invert == 2:
            assert np.array_equal(A, A.T), tag
        A = (np.tril(A) + np.tril(A, -1).T).astype(LD)
        r, bar = _amax(Kl @ A - np.eye(n, dtype=LD)), bar_i
    worst.append(8.0 * r / bar)
    assert r <= bar, (tag, d, r, bar)


def _check_batch(tag, h, K, info, status, invert, which=None):
    """Every problem of ``which`` (default all): info 0, status untouched, the first occurrence of each
    distinct problem against the reference, its repeats against the first occurrence."""
    B = K.shape[0]
    which = range(B) if which is None else which
    first, worst = {}, []
    for b in which:
        assert info[b] == 0 and status[b] == _lib.PQ_UNSOLVED, (tag, b, info[b], status[b])
        d = b % D
        if d in first:
            assert np.array_equal(np.tril(K[b]), np.tril(K[first[d]])), (tag, b, first[d])
            if invert == 2:
                assert np.array_equal(K[b], K[first[d]]), (tag, b)
        else:
            first[d] = b
            _check_problem(tag, h, d, K[b], invert, worst)
    print("KKT %-44s worst 8 x residual / bar %.2f" % (tag, max(worst)))


def _check_untouched(K, Dt, rest):
    for b in rest:
        assert np.isnan(K[b]).all() and np.isnan(Dt[b]).all(), b


# ---- route 0, k_factor -------------------------------------------------------------------------

R0_FACTOR = ([(n, f) for n in (24, 65, 130) for f in FORMS] + [(64, "plain"), (64, "mg4-box-per"), (300, "scaled"),
                                                                  (300, "mg4-box-per")])


@pytest.mark.parametrize("n,form", R0_FACTOR)
def test_route0_factor(device, n, form):
    h = _host(n, form)
    K, Dt, info, status = _run(device, h, 5, 0, ROUTE_GEN)
    _check_batch(f"route0 factor n={n} {form}", h, K, info, status, 0)
    # Dt: the transposed inverses of L's diagonal blocks
    for b in range(5):
        for J in range(K.shape[1] // 64):
            Ljj = np.tril(K[b, 64 * J:64 * J + 64, 64 * J:64 * J + 64])
            r_np = _amax(np.linalg.inv(Ljj).astype(LD) @ Ljj.astype(LD) - np.eye(64))
            assert _amax(Dt[b, J].T.astype(LD) @ Ljj.astype(LD) - np.eye(64)) <= 8.0 * r_np + 1e-15, (b, J)


R0_INVERSE = ([(n, f, inv) for n in (24, 65, 130) for f in ("plain", "mg4-box-per", "mg64-box-shared") for inv in (1, 2)]
              + [(130, "mg1-shared", 1), (130, "box-per", 2), (64, "scaled", 2), (64, "mg4-box-shared", 1),
                 (300, "scaled", 2)])


@pytest.mark.parametrize("n,form,invert", R0_INVERSE)
def test_route0_inverse_large_batch(device, n, form, invert):
    """More problems than CUs: k_factor with its own trtri + lauum (mg = 0 without a box too: beyond the
    resident route's batch bound at ld <= 256, beyond its size at n = 300)."""
    h = _host(n, form)
    B = _cus(device) + 1
    K, Dt, info, status = _run(device, h, B, invert, ROUTE_GEN)
    _check_batch(f"route0 inverse n={n} {form} invert={invert} B={B}", h, K, info, status, invert)


# ---- route 1, k_factor_sk ----------------------------------------------------------------------

R1 = ([(n, f, inv) for n in (65, 130) for f in CONSTRAINED for inv in (1, 2)]
      + [(24, "mg4-box-per", 2), (24, "mg64-box-shared", 1), (64, "mg4-box-per", 1), (64, "box-per", 2),
         (300, "mg4-box-per", 2), (300, "mg64-per", 1)])


@pytest.mark.parametrize("n,form,invert", R1)
def test_route1_inverse(device, n, form, invert):
    h = _host(n, form)
    K, Dt, info, status = _run(device, h, 5, invert, ROUTE_SK)
    _check_batch(f"route1 inverse n={n} {form} invert={invert}", h, K, info, status, invert)


@pytest.mark.parametrize("n,form", [(130, "mg4-box-per"), (65, "mg64-box-shared"), (24, "box-per")])
def test_routes_0_and_1_agree(device, n, form):
    """The same five problems through k_factor (as the head of a batch of CUs + 1) and k_factor_sk."""
    h = _host(n, form)
    K0, _, info0, _ = _run(device, h, _cus(device) + 1, 2, ROUTE_GEN)
    K1, _, info1, _ = _run(device, h, 5, 2, ROUTE_SK)
    assert not info0.any() and not info1.any()
    for b in range(5):
        X = _inverse_ld(h, b)
        d01 = _amax(K0[b, :n, :n] - K1[b, :n, :n])
        d1 = _amax(K1[b, :n, :n].astype(LD) - X)
        print("ROUTES n=%d %s b=%d |K0-K1| %.2e |K1-ref| %.2e" % (n, form, b, d01, d1))
        assert d01 <= 10.0 * d1, (b, d01, d1)


# ---- route 2, k_factor_res: what its own file lacks --------------------------------------------

@pytest.mark.parametrize("n", [65, 284])
@pytest.mark.parametrize("invert", [1, 2])
def test_route2_scaled_form(device, n, invert):
    """ps P + (pd + sigma) I with p_scale, p_diag and sigma all nonzero and distinct per problem."""
    h = _host(n, "scaled")
    K, Dt, info, status = _run(device, h, 5, invert, ROUTE_RES)
    _check_batch(f"route2 inverse n={n} scaled invert={invert}", h, K, info, status, invert)


# ---- pq_factor_large ---------------------------------------------------------------------------

@pytest.mark.parametrize("invert", [0, 2])
@pytest.mark.parametrize("n,form", [(130, f) for f in CONSTRAINED] + [(300, "mg4-box-per"), (300, "mg64-box-shared")])
def test_factor_large_constrained(device, n, form, invert):
    h = _host(n, form)
    idx = [4, 0, 2]
    K, Dt, info, status = _run(device, h, 5, invert, LARGE, idx=idx)
    _check_batch(f"large n={n} {form} invert={invert}", h, K, info, status, invert, which=idx)
    for b in (1, 3):
        assert np.isnan(K[b]).all()


# ---- index lists -------------------------------------------------------------------------------

def test_index_list_route0_more_than_cus(device):
    """nidx > CUs: the list is honoured on k_factor (invert = 1); the problems left out stay NaN."""
    n, form = 65, "mg4-box-per"
    h = _host(n, form)
    cus = _cus(device)
    B = cus + 4
    out = [0, 7, B - 1]
    idx = [b for b in range(B) if b not in out][::-1]
    assert len(idx) > cus
    K, Dt, info, status = _run(device, h, B, 1, ROUTE_GEN, idx=idx)
    _check_batch(f"route0 idx n={n} {form} nidx={len(idx)}", h, K, info, status, 1, which=idx)
    _check_untouched(K, Dt, out)


@pytest.mark.parametrize("route,invert", [(ROUTE_GEN, 0), (ROUTE_SK, 2)])
def test_index_list_subset(device, route, invert):
    n, form = 130, "mg64-per"
    h = _host(n, form)
    K, Dt, info, status = _run(device, h, 5, invert, route, idx=[3, 1])
    _check_batch(f"route{route} idx n={n} {form}", h, K, info, status, invert, which=[3, 1])
    _check_untouched(K, Dt, [0, 2, 4])


# ---- the non-PD contract ------------------------------------------------------------------------

NONPD_C = (0, 15, 16, 63, 64, 129)   # n = 130: problem i's first failing pivot; problems 6, 7 stay PD


@pytest.mark.parametrize("bad", ["negative", "nan"])
@pytest.mark.parametrize("route,form,invert", [(ROUTE_GEN, "mg4-box-per", 0), (ROUTE_SK, "mg4-box-per", 2),
                                               (ROUTE_RES, "scaled", 2), (LARGE, "mg4-box-per", 2)])
def test_non_pd_block_report(device, route, form, invert, bad):
    """K SPD with 2 K[c, c] taken off P[c, c] (the leading c x c minor stays PD: pivot c is the first
    to fail), or a NaN there: info == 1 + 16 (c // 16) and PQ_NON_CONVEX on every route; the other
    problems of the batch are factored / inverted correctly."""
    n = 130
    h = _host(n, form)
    P = h["P"].copy()
    for i, c in enumerate(NONPD_C):
        ps = 1.0 if h["ps"] is None else h["ps"][i]
        P[i, c, c] = np.nan if bad == "nan" else P[i, c, c] - 2.0 * float(_K_ref(h, i)[c, c]) / ps
        if bad == "negative":   # by the reference alone: pivot c is negative, every leading minor before it PD
            Kc = np.asarray(_K_ref(h, i, P[i]), dtype=np.float64)
            assert Kc[c, c] < 0 and (c == 0 or np.linalg.eigvalsh(Kc[:c, :c]).min() > 0)
    K, Dt, info, status = _run(device, h, D, invert, route, P=P)
    want = [1 + 16 * (c // 16) for c in NONPD_C] + [0, 0]
    assert info.tolist() == want, (info.tolist(), want)
    assert np.all(status[:6] == _lib.PQ_NON_CONVEX) and np.all(status[6:] == _lib.PQ_UNSOLVED)
    _check_batch(f"non-PD route {route} {bad}", h, K, info, status, invert, which=[6, 7])
