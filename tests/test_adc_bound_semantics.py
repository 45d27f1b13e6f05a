"""Byte-table ADC prefilter, CPU side: the premise the prefilter stands on, checked on a numpy restatement of
adc_quantise_kernel's arithmetic (tests/adc_bound.py: the same float32 operations in the same order).

Premise: with tau the admission threshold (a float32 ADC distance), every row whose float32 ADC distance is <= tau has
an integer byte-table sum S <= s_tau, so dropping the rows with S > s_tau loses no admissible row.

Domain: the largest subtable range rmax is 0 (constant subtables, S == 0 for every row) or at least
adc_bound.MIN_RANGE = 2^-100, the table has no NaN / negative / infinite entry and tau <= 1e18.  Outside it the kernel
sets ok = 0 and the host serves the query on the exact schedule.  The floor exists because 255 / rmax overflows to +inf
below rmax = 255 / FLT_MAX ~ 7.5e-37: the restatement WITHOUT the floor (floor=None) loses admissible rows there, which
test_overflowing_reciprocal_breaks_the_bound_without_the_floor shows; 2^-100 keeps s = rmax / 255 and 1 / s normal
float32 numbers with margin to spare."""
import numpy as np
import pytest

from oracle import oracle_c as oc
from tests import adc_bound as ab
from tests.adc_bound import family, wrong_survivor_corpus

F = np.float32
FAMILIES = ["uniform", "dominant", "offset", "dyadic", "huge", "tiny"]


def lost_rows(table, codes, rank, floor=ab.MIN_RANGE):
    """(ok, admissible rows the byte bound would drop, rows it passes) with tau = the rank-th smallest distance"""
    d = oc.adc_batch(table.reshape(-1), codes)
    tau = np.sort(d)[rank]
    q, s_tau, ok = ab.quantise(table, tau, floor)
    S = ab.byte_sums(q, codes)
    return ok, int(((d <= tau) & (S > s_tau)).sum()), int((S <= s_tau).sum())


@pytest.mark.parametrize("M", [16, 96])
@pytest.mark.parametrize("name", FAMILIES)
def test_no_admissible_row_is_lost_inside_the_domain(name, M):
    rng = np.random.default_rng(1000 + M + FAMILIES.index(name))
    cb, q = family(name, M, 2, rng)
    codes = rng.integers(0, 256, (20000, M), dtype=np.uint8)
    table = oc.build_adc_table(cb, q).reshape(M, 256)
    for rank in (0, 10, 500, 19999):
        ok, lost, passed = lost_rows(table, codes, rank)
        if name == "tiny":
            assert ok == 0, "a table below the range floor must be refused"
        else:
            assert ok == 1 and lost == 0, (name, M, rank, lost)
            assert passed >= rank + 1


def _unit_table(M, rng):
    t = rng.random((M, 256), dtype=F)
    t[0, 0], t[0, 1] = F(0), F(1)  # largest range exactly 1
    return t


@pytest.mark.parametrize("M", [16, 96])
def test_the_bound_holds_at_the_range_floor_and_is_refused_below_it(M):
    rng = np.random.default_rng(77 + M)
    unit = _unit_table(M, rng)
    codes = rng.integers(0, 256, (20000, M), dtype=np.uint8)
    at = (unit * F(2.0 ** -100)).astype(F)  # power-of-two scaling: exact
    assert ab.minrng(at)[1].max() == ab.MIN_RANGE
    for rank in (0, 10, 500):
        ok, lost, _ = lost_rows(at, codes, rank)
        assert ok == 1 and lost == 0
    below = (unit * F(2.0 ** -101)).astype(F)
    assert lost_rows(below, codes, 10)[0] == 0
    # constant subtables (range 0) stay inside the domain: every S is 0 and every row passes
    const = np.repeat(rng.random((M, 1), dtype=F), 256, axis=1)
    ok, lost, passed = lost_rows(const, codes, 10)
    assert ok == 1 and lost == 0 and passed == 20000


@pytest.mark.parametrize("M", [16, 96])
def test_overflowing_reciprocal_breaks_the_bound_without_the_floor(M):
    rng = np.random.default_rng(99 + M)
    unit = _unit_table(M, rng)
    codes = rng.integers(0, 256, (20000, M), dtype=np.uint8)
    # 2^-120 is below the floor but 255 / rmax is still finite: the arithmetic itself is sound there, the floor is conservative
    ok, lost, _ = lost_rows((unit * F(2.0 ** -120)).astype(F), codes, 500, floor=None)
    assert ok == 1 and lost == 0
    # 2^-125 ~ 2.4e-38 < 255 / FLT_MAX: the reciprocal is +inf and admissible rows are dropped
    small = (unit * F(2.0 ** -125)).astype(F)
    with np.errstate(over="ignore"):
        assert np.isinf(F(255) / ab.minrng(small)[1].max())
    ok, lost, _ = lost_rows(small, codes, 500, floor=None)
    assert ok == 1 and lost > 0
    assert lost_rows(small, codes, 500)[0] == 0  # with the floor the query goes to the exact schedule


def test_wrong_survivors_without_the_floor():
    """the restated search on wrong_survivor_corpus: without the floor at least k rows survive and none is flagged, yet
    the five nearest rows are missing; with the floor the query is refused (ok = 0) and served exactly"""
    n, k = 66001, 10
    cb, q, codes, near = wrong_survivor_corpus(n)
    table = oc.build_adc_table(cb, q).reshape(16, 256)
    d = oc.adc_batch(table.reshape(-1), codes)
    assert set(np.argsort(d, kind="stable")[:5]) == set(near)
    cnt, m, _, cap = ab.plan(n, k)
    assert cnt != 0
    tau = ab.sampled_tau(d, cnt, m)
    qt, s_tau, ok = ab.quantise(table, tau, floor=None)
    surv = (ab.byte_sums(qt, codes) <= s_tau) & (d <= tau)
    assert ok == 1 and k <= surv.sum() <= cap            # nothing tells the select that rows are missing
    assert not surv[near].any()                           # ... but the true nearest rows are
    assert ab.quantise(table, tau)[2] == 0
