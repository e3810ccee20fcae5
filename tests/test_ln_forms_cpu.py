"""CPU tier: the dispatch of rcot_ln_bwd (csrc/pointwise.hip) restated in Python, held against the literals of the case table that
tests/test_ln_forms_gpu.py runs, and rcot_ln_bwd_rows — host-only, it launches nothing — held against the restatement for that table
and for every shape the trainer can produce; those shapes' deferred partial rows must fit HipBackend._ln_scratch."""
import pytest

from ln_forms_cases import CASES, IDS
from rcot_amd import lib
from rcot_amd.ops import LN_SCRATCH_FLOATS

# the trainer: patch sizes 32..1024 in steps of 32, four levels (the plane halves per level), the four widths, its batch sizes
PATCHES = range(32, 1025, 32)
LEVELS = range(4)
WIDTHS = (48, 96, 192, 384)
BATCHES = (1, 2, 3, 4, 6, 8, 16, 32, 64)


def ln_bwd_dispatch(B, C, N):
    """rcot_ln_bwd's choice for [B, C, N]: 64-pixel tiles on 16 x 16 threads (wide) while they give at least 512 workgroups, else
    16-pixel tiles on 64 thread-rows x 4 quads; the channels stay in registers (NC = C / TY) when that quotient is 3 or 6; a grid of
    gx x B workgroups with gx * B <= 1024 where B allows, each walking its tiles in steps of gx and leaving ONE partial row."""
    cdiv = lambda a, b: -(-a // b)
    wide = cdiv(N, 64) * B >= 512
    TX, TY = (16, 16) if wide else (4, 64)
    NC = C // TY if C % TY == 0 and C // TY in (3, 6) else 0
    tiles = cdiv(N, 4 * TX)
    gx = min(max(1024 // B, 1), tiles)
    return dict(wide=wide, TY=TY, NC=NC, TX=TX, tiles=tiles, gx=gx, trips=cdiv(tiles, gx), rows=gx * B)


def _rows(B, C, N):
    return int(lib.load().rcot_ln_bwd_rows(B, C, N))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_table_literals_follow_from_the_rule(case):
    d = ln_bwd_dispatch(case.B, case.C, case.N)
    assert case.kernel == f"ln_bwd_kernel<{d['NC']}, {d['TX']}>", d
    assert (case.tiles, case.gx, case.trips, case.rows) == (d["tiles"], d["gx"], d["trips"], d["rows"]), d
    assert case.N % 4 == 0 and case.C <= 512
    assert _rows(case.B, case.C, case.N) == case.rows


def test_case_table_reaches_every_form_and_every_edge():
    forms = {c.kernel for c in CASES}
    assert forms == {f"ln_bwd_kernel<{nc}, {tx}>" for nc in (0, 3, 6) for tx in (16, 4)}
    for tx, tile in ((16, 64), (4, 16)):
        mine = [c for c in CASES if c.kernel.endswith(f", {tx}>")]
        assert any(c.trips == 2 for c in mine), tx                          # a second trip of the grid-stride loop
        assert any(c.N % tile for c in mine), tx                             # a ragged last tile
    assert any(c.B > 1024 for c in CASES)
    rows = {c.rows for c in CASES}
    assert any(225 <= r <= 256 for r in rows) and any(256 < r <= 288 for r in rows), sorted(rows)   # the reducers' unroll boundaries
    prods = sorted(-(-c.N // 64) * c.B for c in CASES)
    assert 511 in prods and 512 in prods                                    # both sides of the width threshold


def test_rows_of_every_training_shape():
    L = lib.load()
    n = 0
    for P in PATCHES:
        for lv in LEVELS:
            N = (P >> lv) ** 2
            assert N % 4 == 0
            for C in WIDTHS:                 # the trainer ties C = 48 << level; every width at every plane holds a superset
                for B in BATCHES:
                    d = ln_bwd_dispatch(B, C, N)
                    got = int(L.rcot_ln_bwd_rows(B, C, N))
                    assert got == d["rows"], (P, lv, C, B, got, d)
                    assert 0 < got <= 1024, (P, lv, C, B, got)
                    assert got * 2 * C <= LN_SCRATCH_FLOATS, (P, lv, C, B, got)
                    n += 1
    assert n == 32 * 4 * 4 * 9


def test_scratch_constant_keeps_its_value():
    assert LN_SCRATCH_FLOATS == 1024 * 1024


def test_rows_of_nothing():
    assert _rows(0, 48, 64) == 0 and _rows(2, 48, 0) == 0
