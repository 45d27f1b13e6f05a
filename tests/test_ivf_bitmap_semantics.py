"""tests/ivf_bitmap_cases.py pinned on the CPU: the packing is least significant bit first and survives bit lengths that are no
multiple of 8, longbow_amd.ivf.pack_bitmap gives those very bytes, the strided form is one single-bitmap search per query, and the
shapes tests/test_gpu_ivf_bitmap.py relies on are what it takes them for."""
import numpy as np
import pytest

from tests import ivf_bitmap_cases as bc
from tests import ivf_filter_cases as fc
from tests import ivf_oracle as io


@pytest.fixture(scope="module")
def parity(oracle):
    X, Q, C = io.parity_case()
    return X, Q, C, io.assign(oracle, 0, 0, X, C)


def test_packing_is_lsb_first():
    assert bc.pack([1, 0, 0, 0, 0, 0, 0, 0]).tolist() == [0x01]
    assert bc.pack([0, 0, 0, 0, 0, 0, 0, 1]).tolist() == [0x80]
    assert bc.pack([0] * 8 + [1]).tolist() == [0x00, 0x01]
    assert bc.pack([0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]).tolist() == [0x02, 0x04]
    assert bc.pack([0, 7, 0x80, 0xFF]).tolist() == [0x0E]          # any non-zero byte is a set bit, as in the handle filter's mask
    assert bc.pack([]).size == 0
    m = np.zeros(3000, np.uint8)
    m[[0, 9, 2999]] = 1
    b = bc.pack(m)
    assert b.size == 375 and b[0] == 1 and b[1] == 2 and b[374] == 0x80 and np.count_nonzero(b) == 3
    # an Arrow validity buffer is this layout
    assert np.array_equal(b, np.packbits(m, bitorder="little"))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 17, 2999, 3001, 3007])
def test_bit_lengths_that_are_no_multiple_of_eight(n):
    rng = np.random.default_rng(n)
    m = (rng.random(n) < 0.5).astype(np.uint8)
    m[-1] = 1
    b = bc.pack(m)
    assert b.size == bc.nbytes(n) == -(-n // 8)
    assert np.array_equal(bc.unpack(b, n), m)
    if n % 8:
        assert b[-1] >> (n % 8) == 0                                # the bits past n - 1 are zero
    # what lies past bit n - 1 is not looked at: ones there change nothing
    noisy = np.concatenate([b, np.full(3, 0xFF, np.uint8)])
    if n % 8:
        noisy[b.size - 1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    assert np.array_equal(bc.unpack(noisy, n), m)


def test_the_front_end_packs_the_same_bytes():
    from longbow_amd import ivf
    rng = np.random.default_rng(3)
    for n in (1, 9, 3000, 3001):
        m = (rng.random(n) < 0.3).astype(np.uint8) * np.uint8(0x80)  # a byte mask: non-zero is visible
        bits, stride = ivf.pack_bitmap(m)
        assert stride == 0 and bits.dtype == np.uint8 and np.array_equal(bits, bc.pack(m))
        assert np.array_equal(ivf.pack_bitmap(m != 0)[0], bits)      # a bool mask too
    masks = bc.per_query_masks(5, 77)
    bits, stride = ivf.pack_bitmap(masks)
    assert stride == bc.nbytes(77) == 10 and bits.shape == (5, 10) and bits.flags.c_contiguous
    assert np.array_equal(bits, bc.pack_rows(masks))
    with pytest.raises(ValueError):
        ivf.pack_bitmap(np.zeros((2, 2, 2), np.uint8))


def test_pack_rows_strides_and_fill():
    masks = bc.per_query_masks(6, 21)
    assert masks[0].sum() == 0 and masks[1].all() and len({m.tobytes() for m in masks}) == 6
    wide = bc.pack_rows(masks, stride=7, fill=0xFF)
    assert wide.shape == (6, 7) and (wide[:, 3:] == 0xFF).all()
    for q in range(6):
        assert np.array_equal(bc.unpack(wide[q], 21), masks[q])
    with pytest.raises(AssertionError):
        bc.pack_rows(masks, stride=2)


def test_a_bitmap_search_is_the_filtered_search_of_the_unpacked_bits(oracle, parity):
    X, Q, C, lists = parity
    masks = fc.parity_masks()
    for name in ("10 % byte mask", "row 0"):
        want = fc.search_filtered(oracle, 0, 0, Q, X, C, lists, masks[name], fc.K, 3)
        got = bc.search_bitmap(oracle, 0, 0, Q, X, C, lists, bc.pack(masks[name]), fc.K, 3)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), name
    # ANDed with a handle mask: the product of the two
    both = (masks["10 % byte mask"] != 0) & (masks["50 % byte mask"] != 0)
    want = fc.search_filtered(oracle, 0, 0, Q, X, C, lists, both, fc.K, 3)
    got = bc.search_bitmap(oracle, 0, 0, Q, X, C, lists, bc.pack(masks["10 % byte mask"]), fc.K, 3, also=masks["50 % byte mask"])
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_the_stride_form_is_one_single_bitmap_search_per_query(oracle, parity):
    X, Q, C, lists = parity
    n = X.shape[0]
    masks = bc.per_query_masks(Q.shape[0], n)
    bits = bc.pack_rows(masks, stride=bc.nbytes(n) + 5, fill=0xFF)
    lab, dist, scanned = bc.search_strided(oracle, 0, 0, Q, X, C, lists, bits, fc.K, 3)
    for q in range(Q.shape[0]):
        wl, wd, ws = fc.search_filtered(oracle, 0, 0, Q[q:q + 1], X, C, lists, masks[q], fc.K, 3)
        assert np.array_equal(lab[q], wl[0]) and np.array_equal(dist[q], wd[0]) and scanned[q] == ws[0], q
    assert (lab[0] == -1).all() and scanned[0] == 0                  # the all-zero bitmap
    wl, wd, ws = io.search(oracle, 0, 0, Q[1:2], X, C, lists, fc.K, 3)
    assert np.array_equal(lab[1], wl[0]) and scanned[1] == ws[0]     # the all-one bitmap: the plain search


def test_step_edge_case_shape(oracle):
    """list i holds STEP_COUNTS[i] rows and the masks leave it exactly STEP_KEEP[i], first rows or a random choice; query i probes
    list i"""
    X, Q, C, owner = io.edge_case(bc.STEP_COUNTS)
    assert X.shape[0] == sum(bc.STEP_COUNTS) and np.bincount(owner).tolist() == list(bc.STEP_COUNTS)
    assert all(k <= c for k, c in zip(bc.STEP_KEEP, bc.STEP_COUNTS))
    assert np.array_equal(io.assign(oracle, 0, 0, X, C), owner)
    assert [int(io.probes(oracle, 0, 0, Q[i], C, 1)[0]) for i in range(len(bc.STEP_COUNTS))] == list(range(len(bc.STEP_COUNTS)))
    first, rand = fc.keep_per_list(owner, bc.STEP_KEEP), fc.keep_per_list(owner, bc.STEP_KEEP, np.random.default_rng(6))
    for m in (first, rand):
        assert np.bincount(owner[m != 0], minlength=len(bc.STEP_KEEP)).tolist() == list(bc.STEP_KEEP)
        assert np.array_equal(bc.unpack(bc.pack(m), m.size), m)
    assert not np.array_equal(first, rand)
