"""tests/ivf_code_bitmap_cases.py pinned on the CPU: for each of the IVF-PQ handle plain ("pq") and residual ("rpq") and the IVF-SQ8
handle ("sq8"), a search under a call's bitmap is the kind's oracle with the unpacked bits as the mask, ANDed with a handle mask it
is the oracle under the product of the two, with a stride it is one such search per query, on a residual handle the table of a row
is that of the list probed whatever the mask hides, and the shapes tests/test_gpu_ivf_code_bitmap.py relies on are what it takes
them for."""
import numpy as np
import pytest

from tests import ivf_bitmap_cases as bc
from tests import ivf_code_bitmap_cases as kc
from tests import ivf_code_remove_cases as cc
from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io

KINDS = list(cc.KINDS)
F = np.float32


@pytest.mark.parametrize("kind", KINDS)
def test_a_bitmap_search_is_the_oracle_under_the_unpacked_bits_and_the_product_mask(oracle, kind):
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    assert (c.n, c.nlist, c.Q.shape[0]) == (3000, 16, 33)
    masks = fc.parity_masks()
    for name in ("10 % byte mask", "row 0"):
        want = c.search(oracle, c.Q, (masks[name] != 0).astype(np.uint8), kc.K, 3)
        got = kc.search_bitmap(oracle, c, c.Q, bc.pack(masks[name]), kc.K, 3)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (kind, name)
    # unpack(pack(mask)) ANDed with a handle mask: the product of the two
    both = ((masks["10 % byte mask"] != 0) & (masks["50 % byte mask"] != 0)).astype(np.uint8)
    want = c.search(oracle, c.Q, both, kc.K, 3)
    got = kc.search_bitmap(oracle, c, c.Q, bc.pack(masks["10 % byte mask"]), kc.K, 3, also=masks["50 % byte mask"])
    for a, b in zip(got, want):
        assert np.array_equal(a, b), kind
    assert want[2].sum() < c.search(oracle, c.Q, (masks["50 % byte mask"] != 0).astype(np.uint8), kc.K, 3)[2].sum()


@pytest.mark.parametrize("kind", KINDS)
def test_the_stride_form_is_one_single_bitmap_search_per_query(oracle, kind):
    c = cc.parity(oracle, kind, cc.FIRST_SHAPE[kind])
    nq = c.Q.shape[0]
    masks = bc.per_query_masks(nq, c.n)
    bits = bc.pack_rows(masks, stride=bc.nbytes(c.n) + 5, fill=0xFF)
    lab, dist, scanned = kc.search_strided(oracle, c, c.Q, bits, kc.K, 3)
    for q in range(nq):
        wl, wd, ws = c.search(oracle, c.Q[q:q + 1], masks[q], kc.K, 3)
        assert np.array_equal(lab[q], wl[0]) and np.array_equal(dist[q], wd[0]) and scanned[q] == ws[0], (kind, q)
    assert (lab[0] == -1).all() and scanned[0] == 0                  # the all-zero bitmap
    wl, wd, ws = c.search(oracle, c.Q[1:2], np.ones(c.n, np.uint8), kc.K, 3)
    assert np.array_equal(lab[1], wl[0]) and scanned[1] == ws[0]     # the all-one bitmap: the plain search


def test_a_residual_table_is_the_probed_lists_whatever_the_mask_hides(oracle):
    """every distance a masked search reports is ADC under the table of q - C[list of that row], and hiding every row of a query's
    nearest list changes no distance of the rows of its other probed lists"""
    c = cc.parity(oracle, "rpq", cc.FIRST_SHAPE["rpq"])
    nprobe = 3
    mask = (fc.parity_masks()["50 % byte mask"] != 0).astype(np.uint8)
    lab, dist, _ = c.search(oracle, c.Q, mask, kc.K, nprobe)
    for q in range(c.Q.shape[0]):
        pr = io.probes(oracle, 0, 0, c.Q[q], c.C, nprobe)
        for j in np.flatnonzero(lab[q] >= 0):
            r = lab[q, j]
            assert mask[r] and c.lists[r] in pr
            table = oracle.build_adc_table(c.par, (c.Q[q] - c.C[c.lists[r]]).astype(F))
            assert dist[q, j] == oracle.adc_batch(table, c.codes[r:r + 1])[0], (q, j)
    q = 4
    pr = io.probes(oracle, 0, 0, c.Q[q], c.C, nprobe)
    hide_first = (c.lists != pr[0]).astype(np.uint8)
    all_l, all_d, _ = c.search(oracle, c.Q[q:q + 1], np.ones(c.n, np.uint8), c.n, nprobe)
    hid_l, hid_d, hid_s = c.search(oracle, c.Q[q:q + 1], hide_first, c.n, nprobe)
    keep = (all_l[0] >= 0) & (c.lists[np.clip(all_l[0], 0, None)] != pr[0])
    assert hid_s[0] == np.isin(c.lists, pr[1:]).sum() == keep.sum() > 0
    assert np.array_equal(hid_l[0, :keep.sum()], all_l[0][keep]) and np.array_equal(hid_d[0, :keep.sum()], all_d[0][keep])


@pytest.mark.parametrize("kind", KINDS)
def test_step_case_shape(oracle, kind):
    """list i holds STEP_COUNTS[i] rows and the masks leave it exactly STEP_KEEP[i]; query i probes list i; the codes of a list
    differ"""
    c = kc.step_case(oracle, kind)
    assert c.n == sum(bc.STEP_COUNTS) == 16388 and np.bincount(c.lists).tolist() == list(bc.STEP_COUNTS)
    assert np.array_equal(c.k.assign(oracle, c.X, c.C), c.lists)
    assert [int(io.probes(oracle, 0, 0, c.Q[i], c.C, 1)[0]) for i in range(c.nlist)] == list(range(c.nlist))
    for l in range(1, c.nlist):
        assert np.unique(c.codes[c.lists == l], axis=0).shape[0] > 1, (kind, l)
    first, rand = fc.keep_per_list(c.lists, bc.STEP_KEEP), fc.keep_per_list(c.lists, bc.STEP_KEEP, np.random.default_rng(6))
    for m in (first, rand):
        assert np.bincount(c.lists[m != 0], minlength=c.nlist).tolist() == list(bc.STEP_KEEP)
        assert kc.search_bitmap(oracle, c, c.Q, bc.pack(m), kc.K, 1)[2].tolist() == list(bc.STEP_KEEP)


def test_which_form_each_shape_of_the_gpu_tests_takes(oracle):
    """the host's rule restated (ivf_code_bitmap_cases.shared_form) on the shapes tests/test_gpu_ivf_code_bitmap.py names"""
    c = cc.parity(oracle, "pq", cc.FIRST_SHAPE["pq"])
    sizes = np.bincount(c.lists, minlength=c.nlist)
    assert not kc.shared_form(sizes, 1, 1, 0)            # one query, one probe: at most the largest list, fewer than all rows
    assert kc.shared_form(sizes, 33, 16, 0)              # 33 queries x all 3,000 rows
    assert not kc.shared_form(sizes, 33, 16, 375)        # a bitmap per query: never
    s = cc.skew(oracle, "pq")
    ssz = np.bincount(s.lists, minlength=s.nlist)
    assert ssz[0] > 2 * fc.LDS_KEYS and s.Q.shape[0] == 8 and kc.shared_form(ssz, 8, 1, 0)   # 8 x ~37,000 > 50,000
    assert not kc.shared_form(ssz, 1, 1, 0)
    st = np.asarray(bc.STEP_COUNTS)
    assert kc.shared_form(st, 6, 1, 0) and not kc.shared_form(st, 1, 1, 0) and not kc.shared_form(st, 2, 1, 0)  # 2 x 6,144 < 16,388
    assert kc.shared_form(np.zeros(4, np.int64), 1, 1, 0)  # nothing visible: one step over nothing
