"""GPU tier: every form of the LayerNorm backward (rcot_ln_bwd of csrc/pointwise.hip: ln_bwd_kernel<NC, TX>, six instantiations) and its
two reducers (ln_param_reduce_kernel, the LayerNorm part of block_param_reduce_kernel), branch by branch, at the smallest shape that
reaches the branch — the companion of tests/test_conv_dispatch_gpu.py and tests/test_gemm_dispatch_gpu.py for this kernel.

The cases and their hand-derived form, tile count, grid, trips and partial rows are the literals of tests/ln_forms_cases.py (the CPU
tier holds them against a restatement of the dispatch rule).  Every case goes through HipBackend.ln_stats and HipBackend.ln_bwd on
guard-banded buffers (tests/guarded.py) with NaN-filled outputs and NaN-filled workspaces, in two routes:
  immediate  dres given, dw / db given: ln_param_reduce_kernel adds the partial rows of the workspace up in the same call;
  deferred   dres given, slot = 0 (and the same call again into slot 1): the partial rows stay in the backend's LN scratch and
             block_param_reduce adds them up — the combination the network runs;
and asserts
  * the kernel that ran (rcot_last_kernel) against the symbol written in the table, and that the count moved by one per call,
  * mu, rs and dx against the fp64 double (tests/host_double.py) at TOL (2e-5 of max|ref|), dw and db at 1e-4 (test_block_param_reduce's
    bar for sums over batch and plane),
  * the partial rows: exactly rcot_ln_bwd_rows(B, C, N) * 2 C leading floats of the workspace / scratch slot are finite, the rest NaN,
  * every output finite, every guard band intact.
The deferred route writes slot 1 from identical inputs: dx, the partial rows and the reduced dw / db of the two slots must agree bit
for bit (each form promises a fixed summation order; test_two_runs_agree_bit_for_bit repeats that across whole runs, both routes).

Every case prints an LN-BWD-FORM line before it asserts (profiles/ln_bwd_forms.txt)."""
import time

import pytest
import torch

from conftest import relerr
from guarded import GuardSet, all_finite, poison_workspaces
from ln_forms_cases import BY_NAME, CASES, IDS
from rcot_amd import lib as _lib
from rcot_amd.lib import RcotKernelError
from test_kernels_gpu import DBL, TOL, _last_kernel, hip  # noqa: F401  (hip: the module-scoped backend fixture)

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-4        # dw, db: sums over batch and plane (the bar of test_block_param_reduce)
NAN = float("nan")
ROUTES = ["immediate", "deferred"]
HEADS = 2             # block_param_reduce also sums dW_o and the temperature partials: small ones ride along and are checked


def _seq(be):
    return be.L.rcot_last_kernel(None, 0)


# ----------------------------------------------------------------------------- inputs and the fp64 reference, once per shape
_made = {}


def _problem(case, with_dres=True):
    """fp32 host inputs of a case and its fp64 results; the last one made is kept (the routes of a case run back to back)"""
    key = (case.name, with_dres)
    if key in _made:
        return _made[key]
    _made.clear()
    B, C, N = case.B, case.C, case.N
    gen = torch.Generator().manual_seed(7919 * B + 31 * C + N)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    p = dict(x=rn(B, C, N) + 0.5, g=rn(B, C, N), w=1 + 0.1 * rn(C), dres=rn(B, C, N) if with_dres else None, dw0=rn(C), db0=rn(C),
             dWp=rn(B, C, C), gWo0=rn(C, C), dtp=rn(B, HEADS), gtemp0=rn(HEADS))
    d = lambda t: None if t is None else t.double()
    mu, rs = torch.zeros(B, N, dtype=torch.float64), torch.zeros(B, N, dtype=torch.float64)
    dx = torch.zeros(B, C, N, dtype=torch.float64)
    dw, db = p["dw0"].double(), p["db0"].double()
    DBL.ln_stats(d(p["x"]), mu, rs)
    DBL.ln_bwd(d(p["g"]), d(p["x"]), mu, rs, d(p["w"]), d(p["dres"]), dx, dw, db)
    p["ref"] = dict(mu=mu, rs=rs, dx=dx, dw=dw, db=db, gWo=p["gWo0"].double() + p["dWp"].double().sum(0),
                    gtemp=p["gtemp0"].double() + p["dtp"].double().sum(0))
    _made[key] = p
    return p


def _upload(gs, p, case, names=("x", "g", "w", "dres")):
    B, N = case.B, case.N
    t = {n: (None if p[n] is None else gs.tensor(p[n], n)) for n in names}
    t["mu"], t["rs"] = gs.full((B, N), NAN, name="mu"), gs.full((B, N), NAN, name="rs")
    return t


def _partial_rows_ok(buf, live):
    """exactly the first ``live`` floats of a NaN-filled buffer were written, with finite values"""
    return bool(torch.isfinite(buf[:live]).all()) and bool(torch.isnan(buf[live:]).all())


def _run_immediate(be, gs, p, case, t):
    """ln_stats + ln_bwd with dw / db given; returns (symbol, launches noted, dx, dw, db, partial rows)"""
    B, C, N = case.B, case.C, case.N
    dx = gs.full((B, C, N), NAN, name="dx")
    dw, db = gs.tensor(p["dw0"], "dw"), gs.tensor(p["db0"], "db")
    poison_workspaces(be)
    be.ln_stats(t["x"], t["mu"], t["rs"])
    s0 = _seq(be)
    be.ln_bwd(t["g"], t["x"], t["mu"], t["rs"], t["w"], t["dres"], dx, dw, db)
    sym, noted = _last_kernel(be), _seq(be) - s0
    torch.cuda.synchronize()
    return sym, noted, dx, dw, db, be.ws


def _run_deferred(be, gs, p, case, t):
    """ln_stats, ln_bwd into slot 0 and again into slot 1, the scratch read BEFORE block_param_reduce; returns
    (symbol, launches noted, (dx, dx'), (scratch 0, scratch 1) as they were before the reduce, reduced gradients)"""
    B, C, N = case.B, case.C, case.N
    dx, dx2 = gs.full((B, C, N), NAN, name="dx"), gs.full((B, C, N), NAN, name="dx (slot 1)")
    out = {n: gs.tensor(p[src], n) for n, src in (("gw1", "dw0"), ("gb1", "db0"), ("gw2", "dw0"), ("gb2", "db0"), ("gWo", "gWo0"),
                                                  ("gtemp", "gtemp0"))}
    dWp, dtp = gs.tensor(p["dWp"], "dWo_part"), gs.tensor(p["dtp"], "dtemp_part")
    poison_workspaces(be)
    be.ln_stats(t["x"], t["mu"], t["rs"])
    gen, s0 = be._gen, _seq(be)
    be.ln_bwd(t["g"], t["x"], t["mu"], t["rs"], t["w"], t["dres"], dx, None, None, slot=0)
    sym, noted = _last_kernel(be), _seq(be) - s0
    be.ln_bwd(t["g"], t["x"], t["mu"], t["rs"], t["w"], t["dres"], dx2, None, None, slot=1)
    sym2 = _last_kernel(be)
    torch.cuda.synchronize()
    assert sym2 == sym and be._gen == gen
    sc = [be._ln_scratch[gen][s].clone() for s in (0, 1)]
    be.block_param_reduce(C, out["gw1"], out["gb1"], out["gw2"], out["gb2"], dWp, out["gWo"], dtp, out["gtemp"])
    torch.cuda.synchronize()
    return sym, noted, (dx, dx2), sc, out


def _record(case, route, sym, errs, t0, note=""):
    print(f"LN-BWD-FORM ({case.B},{case.C},{case.N}) {route}{note}: {sym} tiles={case.tiles} gx={case.gx} trips={case.trips} "
          f"rows={case.rows} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items())
          + f" bar={TOL:g}/{SUM_TOL:g} wall={1e3 * (time.perf_counter() - t0):.0f}ms")


def _check_case(be, case, route, with_dres=True):
    t0 = time.perf_counter()
    p = _problem(case, with_dres)
    ref, live = p["ref"], case.rows * 2 * case.C
    assert int(be.L.rcot_ln_bwd_rows(case.B, case.C, case.N)) == case.rows
    gs = GuardSet("cuda")
    t = _upload(gs, p, case)
    if route == "immediate":
        sym, noted, dx, dw, db, part = _run_immediate(be, gs, p, case, t)
        rows_ok, outs, same = _partial_rows_ok(part, live), [dx, dw, db], True
    else:
        sym, noted, (dx, dx2), sc, out = _run_deferred(be, gs, p, case, t)
        dw, db = out["gw1"], out["gb1"]
        rows_ok = _partial_rows_ok(sc[0], live) and _partial_rows_ok(sc[1], live)
        same = (torch.equal(dx, dx2) and torch.equal(sc[0][:live], sc[1][:live]) and torch.equal(out["gw1"], out["gw2"])
                and torch.equal(out["gb1"], out["gb2"]))
        outs = [dx, dx2, *out.values()]
    errs = {"mu": relerr(t["mu"], ref["mu"]), "rs": relerr(t["rs"], ref["rs"]), "dx": relerr(dx, ref["dx"]),
            "dw": relerr(dw, ref["dw"]), "db": relerr(db, ref["db"])}
    _record(case, route, sym, errs, t0, "" if with_dres else " dres=None")
    assert sym == case.kernel and noted == 1, (sym, noted)
    assert max(errs["mu"], errs["rs"], errs["dx"]) < TOL, errs
    assert max(errs["dw"], errs["db"]) < SUM_TOL, errs
    if route == "deferred":
        e = {"gWo": relerr(out["gWo"], ref["gWo"]), "gtemp": relerr(out["gtemp"], ref["gtemp"])}
        assert max(e.values()) < SUM_TOL, e
    assert rows_ok, f"not exactly the first {live} floats of the partial rows were written"
    assert same, "slot 1 differs from slot 0 on identical inputs"
    assert all(all_finite(o) for o in [t["mu"], t["rs"], *outs])
    gs.check()


# ----------------------------------------------------------------------------- every form, both routes
# (the upper decorator varies fastest: the two routes of a case run back to back and share one fp64 reference)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_form(hip, case, route):
    _check_case(hip, case, route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ["wide-regs-3", "narrow-generic"])
def test_form_without_a_residual(hip, name, route):
    """dres = None: dx is the LayerNorm's own gradient, nothing is read through the null pointer"""
    _check_case(hip, BY_NAME[name], route, with_dres=False)


# ----------------------------------------------------------------------------- determinism: one case per form, whole runs repeated
# the two-trip / ragged / many-row member of every form where the table has one (the order ACROSS a workgroup's tiles is part of the promise)
DETERMINISM = ["wide-ragged-tile", "wide-two-trips-one-workgroup", "wide-generic-c100", "reducer-258-rows", "reducer-240-rows",
               "threshold-511-narrow"]


@pytest.mark.parametrize("name", DETERMINISM)
@pytest.mark.parametrize("route", ROUTES)
def test_two_runs_agree_bit_for_bit(hip, name, route):
    case = BY_NAME[name]
    live = case.rows * 2 * case.C
    B, C, N = case.B, case.C, case.N
    gen = torch.Generator().manual_seed(104729 + C + N)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    p = dict(x=rn(B, C, N) + 0.5, g=rn(B, C, N), w=1 + 0.1 * rn(C), dres=rn(B, C, N), dw0=rn(C), db0=rn(C), dWp=rn(B, C, C),
             gWo0=rn(C, C), dtp=rn(B, HEADS), gtemp0=rn(HEADS))
    gs = GuardSet("cuda")
    t = _upload(gs, p, case)
    got = []
    for _ in range(2):
        if route == "immediate":
            sym, _, dx, dw, db, part = _run_immediate(hip, gs, p, case, t)
            got.append((sym, dx, part[:live].clone(), dw, db))
        else:
            sym, _, (dx, _dx2), sc, out = _run_deferred(hip, gs, p, case, t)
            got.append((sym, dx, sc[0][:live], out["gw1"], out["gb1"]))
    (sa, *a), (sb, *b) = got
    assert sa == sb == case.kernel
    for what, u, v in zip(("dx", "partial rows", "dw", "db"), a, b):
        assert all_finite(u) and torch.equal(u, v), f"{what} differs between two runs of {case.kernel} ({route})"
    gs.check()


# ----------------------------------------------------------------------------- channel isolation
# (case, c0): c0 belongs to the LAST thread-row (ty = TY - 1 owns channels TY - 1, 2 TY - 1, ...), in its last register / last trip
ISOLATION = [("wide-regs-6-threshold-512", 95),       # TY = 16, NC = 6: thread-row 15, register 5
             ("wide-generic-c100", 95),               # TY = 16, generic: thread-row 15's sixth and last channel (96..99 go to rows 0..3)
             ("narrow-regs-3", 191)]                  # TY = 64, NC = 3: thread-row 63, register 2


@pytest.mark.parametrize("name,c0", ISOLATION, ids=[n for n, _ in ISOLATION])
@pytest.mark.parametrize("route", ROUTES)
def test_a_channel_without_gradient_gets_exactly_zero(hip, name, c0, route):
    """g[:, c0] = 0 and dw = db = 0 at the start: every term of dw[c0] and db[c0] is an exact zero, so anything else there came from
    another channel — a leak far below what a bar relative to max|dw| can see"""
    case = BY_NAME[name]
    B, C, N = case.B, case.C, case.N
    gen = torch.Generator().manual_seed(1299709 + C + N)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    z = torch.zeros(C)
    p = dict(x=rn(B, C, N) + 0.5, g=rn(B, C, N), w=1 + 0.1 * rn(C), dres=rn(B, C, N), dw0=z, db0=z, dWp=rn(B, C, C), gWo0=rn(C, C),
             dtp=rn(B, HEADS), gtemp0=rn(HEADS))
    p["g"][:, c0] = 0.0
    gs = GuardSet("cuda")
    t = _upload(gs, p, case)
    if route == "immediate":
        sym, _, dx, dw, db, _part = _run_immediate(hip, gs, p, case, t)
    else:
        sym, _, (dx, _dx2), _sc, out = _run_deferred(hip, gs, p, case, t)
        dw, db = out["gw1"], out["gb1"]
    assert sym == case.kernel
    dw, db = dw.cpu(), db.cpu()
    assert float(dw[c0]) == 0.0 and float(db[c0]) == 0.0, (float(dw[c0]), float(db[c0]))
    others = torch.arange(C) != c0
    assert bool((dw[others] != 0).all()) and bool((db[others] != 0).all())      # the zero is the channel's, not the launch's
    assert all_finite(dx) and all_finite(dw) and all_finite(db)
    gs.check()


# ----------------------------------------------------------------------------- refusals
def _raw_ln_bwd(be, t, dres, dx, dw, db, B, C, N, ws, ws_bytes):
    p = lambda v: None if v is None else v.data_ptr()
    _lib.check(be.L.rcot_ln_bwd(t["g"].data_ptr(), t["x"].data_ptr(), t["mu"].data_ptr(), t["rs"].data_ptr(), t["w"].data_ptr(), p(dres),
                                dx.data_ptr(), p(dw), p(db), B, C, N, ws.data_ptr(), ws_bytes, be._st()), "rcot_ln_bwd")


def _refusal_setup(gs, B, C, N):
    gen = torch.Generator().manual_seed(15485863 + C + N)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32)
    t = {n: gs.tensor(v, n) for n, v in (("x", rn(B, C, N) + 0.5), ("g", rn(B, C, N)), ("w", 1 + 0.1 * rn(C)), ("dres", rn(B, C, N)),
                                         ("mu", rn(B, N)), ("rs", 1 + rn(B, N).abs()), ("dw", rn(C)), ("db", rn(C)))}
    t["dx"] = gs.full((B, C, N), NAN, name="dx")
    return t


REFUSALS = ["C=513", "N=6", "dw-without-db", "dres-off-16-bytes", "workspace-one-byte-short"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(hip, what):
    """RcotKernelError naming rcot_ln_bwd; nothing is launched: dx stays NaN, the last kernel and its count stay, every band stays.
    The workspace case then runs with exactly the bytes it needs, in a guarded buffer of that size: taken, and no row past its end."""
    be = hip
    B, C, N = {"C=513": (1, 513, 16), "N=6": (2, 48, 6)}.get(what, (2, 48, 64))
    gs = GuardSet("cuda")
    t = _refusal_setup(gs, B, C, N)
    need = int(be.L.rcot_ln_bwd_rows(B, C, N)) * 2 * C * 4
    poison_workspaces(be)
    dw0, db0 = t["dw"].clone(), t["db"].clone()
    before = _last_kernel(be), _seq(be)
    with pytest.raises(RcotKernelError, match="rcot_ln_bwd"):
        if what in ("C=513", "N=6"):
            be.ln_bwd(t["g"], t["x"], t["mu"], t["rs"], t["w"], t["dres"], t["dx"], t["dw"], t["db"])
        elif what == "dw-without-db":
            _raw_ln_bwd(be, t, t["dres"], t["dx"], t["dw"], None, B, C, N, be.ws, be.ws_bytes)
        elif what == "dres-off-16-bytes":
            buf = gs.full((B * C * N + 1,), NAN, name="dres + 1 float")
            off = buf[1:].view(B, C, N)
            off.copy_(t["dres"])
            assert off.is_contiguous() and off.data_ptr() % 16 == 4
            be.ln_bwd(t["g"], t["x"], t["mu"], t["rs"], t["w"], off, t["dx"], t["dw"], t["db"])
        else:
            _raw_ln_bwd(be, t, t["dres"], t["dx"], t["dw"], t["db"], B, C, N, be.ws, need - 1)
    torch.cuda.synchronize()
    assert (_last_kernel(be), _seq(be)) == before
    assert bool(torch.isnan(t["dx"]).all()) and not bool(torch.isfinite(be.ws).any())
    assert torch.equal(t["dw"], dw0) and torch.equal(t["db"], db0)
    gs.check()
    if what == "workspace-one-byte-short":
        ws = gs.full((need // 4,), NAN, name="workspace of exactly the bytes needed")
        _raw_ln_bwd(be, t, t["dres"], t["dx"], t["dw"], t["db"], B, C, N, ws, need)
        torch.cuda.synchronize()
        assert _seq(be) == before[1] + 1 and all_finite(ws) and all_finite(t["dx"])
        gs.check()
