"""What a filtered ADC search over PQ codes must return, pinned on the CPU before the GPU is asked: on the inputs of
tests/pq_filter_cases.py the oracle on the visible subset (subset_search, the expected result of tests/test_gpu_pq_filters.py)
agrees with an independent statement, the full ADC distance row with the hidden rows at +inf and a stable argsort.  The
preconditions the GPU cases rely on (visible counts, the decreasing distances of the safe-schedule corpus, the positions of the
duplicate block) are verified here, where the oracle runs."""
import numpy as np
import pytest

from tests import adc_bound as ab
from tests import code_filter_cases as cf
from tests import pq_filter_cases as pc


def _agree(oracle, cb, codes, Q, mask, k, ctx):
    lab, dist = pc.subset_search(oracle, cb, codes, Q, mask, k)
    wlab, wdist = pc.masked_topk(oracle, cb, codes, Q, mask, k)
    assert np.array_equal(lab, wlab) and np.array_equal(dist, wdist), ctx
    vis = np.flatnonzero(mask)
    have = min(k, vis.size)  # the visible rows first, then padding; labels are corpus rows
    assert (lab[:, have:] == -1).all() and (dist[:, have:] == pc.FLT_MAX).all(), ctx
    assert np.isin(lab[:, :have], vis).all(), ctx
    return lab, dist


@pytest.mark.parametrize("k", (1, 10, 100))
@pytest.mark.parametrize("dims,M", pc.SHAPES)
def test_one_boot_chunk_inputs(oracle, dims, M, k):
    cb, codes, Q = pc.corpus(dims, M, pc.N)
    rng = np.random.default_rng(dims + k)
    for name, mask in cf.masks(pc.N, k, rng).items():
        _agree(oracle, cb, codes, Q, mask, k, (name, dims, M, k))
    if (dims, M) in pc.FEW:
        assert set(np.unique(codes)) == set(pc.FEW_VALUES.tolist())


@pytest.mark.parametrize("dims,M", pc.FEW)
def test_several_chunks_inputs(oracle, dims, M):
    cb, codes, Q = pc.corpus(dims, M, pc.N_CHUNKS, nq=3)
    mask = pc.half_mask(pc.N_CHUNKS)
    assert pc.BOOT_POSITIONS < np.count_nonzero(mask) < 65536  # more than the boot chunk, no sampled plan
    assert ab.plan(int(np.count_nonzero(mask)), 300)[0] == 0
    for k in (10, 300):
        _agree(oracle, cb, codes, Q, mask, k, (dims, M, k))


@pytest.mark.parametrize("M", (16, 5))
def test_safe_schedule_corpus_has_strictly_decreasing_distances(oracle, M):
    cb, codes, Q, mask = pc.case_c(M)
    vis = np.flatnonzero(mask)
    assert vis.size == 20_000 and ab.plan(vis.size, 100)[0] == 0
    for q in Q:
        d = oracle.adc_batch(oracle.build_adc_table(cb, q), codes)
        assert (np.diff(d[vis]) < 0).all() and (np.diff(d) < 0).all()
    lab, _ = _agree(oracle, cb, codes, Q, mask, 100, M)
    assert np.array_equal(lab[0], vis[::-1][:100])  # the last visible rows, the nearest first
    # the chunk behind the boot chunk runs to the end of the list and holds more positions than the list has entries
    cap = ab.plan(vis.size, 100)[3]
    assert cap == pc.BOOT_POSITIONS and vis.size - pc.BOOT_POSITIONS > cap


@pytest.mark.parametrize("dims,M", ((32, 16), (768, 96), (60, 5)))
def test_sampled_plan_inputs(oracle, dims, M):
    cb, codes, Q = pc.corpus(dims, M, pc.N_BIG)
    for name, mask in (("half", pc.half_mask(pc.N_BIG)), ("thirds", pc.third_mask(pc.N_BIG))):
        nvis = int(np.count_nonzero(mask))
        assert nvis >= 65536 and ab.plan(nvis, 100)[0] != 0, name  # the sampled plan serves k = 100
        _agree(oracle, cb, codes, Q, mask, 100, (name, dims, M))
    if (dims, M) == (32, 16):
        mask = pc.half_mask(pc.N_BIG)
        assert ab.plan(int(np.count_nonzero(mask)), 1500)[0] == 0  # beyond what sampling supports at this size
        _agree(oracle, cb, codes, Q[:2], mask, 1500, "k 1500")


def test_ties_at_the_sampled_size(oracle):
    cb, codes, Q, mask = pc.case_e()
    assert np.count_nonzero(mask) >= 65536 and np.unique(codes, axis=0).shape[0] == 50
    lab, dist = _agree(oracle, cb, codes, Q, mask, 100, "ties")
    assert (dist == dist[:, :1]).all()  # each query's hundred nearest are copies of one code: the lowest visible rows of it
    assert (np.diff(lab, axis=1) > 0).all()


@pytest.mark.parametrize("dims,M", ((32, 16), (60, 5)))
def test_duplicate_block_positions(oracle, dims, M):
    for boundary in sorted({64, pc.list_waves() * 64}):
        cb, codes, Q, mask, block = pc.case_f(dims, M, boundary)
        vis = np.flatnonzero(mask)
        assert vis.size > boundary + 6
        assert block[5] == vis[boundary - 1] and block[6] == vis[boundary] and block.size == 12
        span = np.arange(block[0], block[-1] + 1)
        assert (mask[span] == 0).sum() >= 5 and (codes[span] == codes[block[0]]).all()
        assert (codes == codes[block[0]]).all(axis=1).sum() == span.size  # no other row equals it
        for k in (6, 12, 20):
            lab, dist = _agree(oracle, cb, codes, Q, mask, k, (dims, M, boundary, k))
            m = min(k, 12)
            assert np.array_equal(lab[0, :m], block[:m]) and (dist[0, :m] == 0).all()
            assert (dist[0, m:] > 0).all()


def test_degenerate_tables_inputs(oracle):
    cb0, cb, codes, Q, mask = pc.case_g()
    vis = np.flatnonzero(mask)
    assert vis.size >= 65536
    lab, dist = _agree(oracle, cb0, codes, Q[:1], mask, 10, "constant tables")
    assert np.array_equal(lab[0], vis[:10]) and len(np.unique(dist)) == 1
    _agree(oracle, cb, codes, Q[:1], mask, 10, "random tables")
    # the query with an infinite component: every distance is +inf, the lowest visible rows win (subset statement alone: the
    # +inf that hides a row in the matrix statement cannot be told from such a distance)
    lab, dist = pc.subset_search(oracle, cb, codes, Q[1:], mask, 10)
    assert np.array_equal(lab[0], vis[:10]) and np.isinf(dist).all()
    # every visible row passes a byte bound over constant tables: more candidates than the buffer holds
    assert vis.size > ab.CAND_CAP


def test_mask_bytes_other_than_one_are_visible(oracle):
    cb, codes, Q = pc.corpus(32, 16, pc.N)
    mask = np.array([0, 1, 2, 0x80, 0xFF, 0], np.uint8)
    lab, _ = pc.subset_search(oracle, cb, codes[:6], Q[:1], mask, 6)
    assert sorted(lab[0][lab[0] >= 0].tolist()) == [1, 2, 3, 4] and (lab[0, 4:] == -1).all()
