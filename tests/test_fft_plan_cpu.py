"""CPU tier: rcot_fft_plan — the host-only entry that decides how rcot_ot_spectrum's line FFT transforms a length (the
dispatcher inside the library calls the same function) — over its whole domain, and the trainer's patch-size check."""
import ctypes

import pytest

from rcot_amd import lib
from rcot_amd.trainer import check_patch_size

RADICES = {2, 3, 4, 5, 7, 11, 13}
CAP = 10


def _plan(n, cap=CAP):
    rad = (ctypes.c_int * max(cap, 1))(*([-7] * max(cap, 1)))
    rc = lib.load().rcot_fft_plan(n, ctypes.cast(rad, ctypes.c_void_p), cap)
    return rc, list(rad)


def _largest_prime_factor(n):
    p, big = 2, 1
    while n > 1:
        while n % p == 0:
            big, n = p, n // p
        p += 1
    return big


def test_every_length_has_a_valid_plan():
    for n in range(2, 1025):
        ns, rad = _plan(n)
        smooth = _largest_prime_factor(n) <= 13
        assert (ns > 0) == smooth, (n, ns)                      # Bluestein exactly when a prime factor exceeds 13
        if ns > 0:
            assert ns <= CAP and set(rad[:ns]) <= RADICES, (n, rad[:ns])
            prod = 1
            for r in rad[:ns]:
                prod *= r
            assert prod == n, (n, rad[:ns])
            assert rad[ns:] == [-7] * (CAP - ns), (n, rad)       # nothing written past the stages
        else:
            assert ns == 0, (n, ns)
            M = rad[0]
            assert M & (M - 1) == 0 and 2 * n - 1 <= M <= 2048, (n, M)
            assert M < 2 * (2 * n - 1), (n, M)                   # the NEXT power of two, not a larger one


def test_powers_of_two_get_their_radix2_plan():
    for k in range(1, 11):
        ns, rad = _plan(1 << k)
        assert ns == k and rad[:k] == [2] * k, (k, ns, rad)


def test_radix_order_four_then_two_then_odd():
    order = [4, 2, 3, 5, 7, 11, 13]
    for n in (96, 160, 224, 352, 1000, 6, 10, 24, 200, 486, 832):
        ns, rad = _plan(n)
        pos = [order.index(r) for r in rad[:ns]]
        assert pos == sorted(pos), (n, rad[:ns])
        assert rad[:ns].count(2) <= 1, (n, rad[:ns])            # radix 4 as often as possible
    assert _plan(96)[1][:4] == [4, 4, 2, 3]
    assert _plan(160)[1][:4] == [4, 4, 2, 5]
    assert _plan(544) == (0, [2048] + [-7] * (CAP - 1))
    assert _plan(136)[1][0] == 512


def test_lengths_outside_the_domain_are_errors():
    assert _plan(1)[0] == -1 and _plan(0)[0] == -1 and _plan(-5)[0] == -1      # RCOT_EINVAL
    assert _plan(1025)[0] == lib.EUNSUPPORTED and _plan(4096)[0] == lib.EUNSUPPORTED
    assert lib.load().rcot_fft_plan(96, None, CAP) == -1
    assert _plan(96, cap=2)[0] == -1                                           # four stages do not fit


def test_plan_entry_is_host_only_for_the_launch_recorder():
    from rcot_amd.plan import _HOST_ONLY
    assert "rcot_fft_plan" in _HOST_ONLY


@pytest.mark.parametrize("P", [32, 96, 160, 1024])
def test_check_patch_size_accepts(P):
    assert check_patch_size(P) == P


@pytest.mark.parametrize("P", [40, 16, 1056])
def test_check_patch_size_rejects(P):
    with pytest.raises(ValueError) as e:
        check_patch_size(P)
    msg = str(e.value)
    assert str(P) in msg and "multiple of 32" in msg and "1024" in msg and "stride-2" in msg and "fc" in msg


def test_cli_refuses_a_bad_patch_size_before_building_anything():
    from rcot_amd import trainer
    saved = trainer.opt
    try:
        with pytest.raises(SystemExit) as e:
            trainer.main(["--synthetic", "--patch_size", "40"])
    finally:
        trainer.opt = saved
    assert "multiple of 32" in str(e.value)
