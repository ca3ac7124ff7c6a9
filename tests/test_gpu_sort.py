"""The argsort kernels of d3d_amd/csrc/sort.hip (k_sort_small, k_ss_*, k_rs_*, k_cs_*; lds_sort.hpp sort_lds<1 / 2>) through
the raw C entries -- d3d_argsort_desc (fp32, fp64), d3d_internal_argsort_desc_radix, d3d_internal_argsort_desc_i32 and
d3d_internal_argsort_desc_counts_dev -- against expected_order() of tests/sort_reference.py: the whole permutation, entry by
entry, no tolerance.  Every call runs in exactly the bytes its size query returns, followed by 64 KiB of 0xA5 that must come
back untouched, on a poisoned `order`, and returns 0.  What a crafted input reaches cannot be seen from outside, so each case
asserts its premise through the model before it launches (tests/test_sort_reference.py holds the model without a GPU).

What each test reaches that the suite did not:
  test_boundary_sizes_every_entry   the int32 keys and int32 order of the i32 entry on all three routes (INT_MIN, INT_MAX, -1,
                                    0, negatives), and for every key type: 64 / 65 (one register run, the first merge pass of
                                    sort_lds), 1024 / 1025 (sort_lds<1> / <2>), 2048 / 2049 (the last one-workgroup sort, the
                                    first sample sort: strata of 2 keys, B = 16), 3071 (1023 keys behind the last stratum of 2),
                                    98303 / 98304 (B = 511 / 512), 131071 .. 131073 (the last sample sorts, the first radix
                                    sort); the radix entry at 1, 64 and around its tiles of 4096.  Known from the constants
                                    that test_sort_reference.py reads out of the source.
  test_oversized_bucket             the fallback of k_ss_bucket (m > kSsBucketCap: 2049, 2112, two buckets of ~3600, one of
                                    15373 entries), the largest bucket still sorted in LDS (2048), sort_lds<2> inside a bucket
                                    (2048; two of ~1580), first and last bucket, NaN inside a pile.  Known from bucket_sizes().
  test_radix_live_passes            every plan of k_rs_plan with one live pass (it reads the caller's keys and writes `order`),
                                    with 0, 2, 3 and all passes live (odd and even: both ends of the ping-pong), a last live
                                    pass below the top byte; fp32 and fp64 through the radix entry, int32 at 131073 keys.
                                    Known from live_bytes().  Runs of 64 equal keys, aligned and shifted by 32, at n % 64 = 1:
                                    both sides of the wavefront-uniform branch of k_rs_hist and a wavefront of one lane.  Known
                                    from wavefront_uniformity().
  test_counts_device_size           k_cs_* on a device-side size of 0, 1, 4095 .. 4097 and n, and NULL; garbage keys behind it;
                                    23 launched tiles beyond it; the second chunk of k_cs_rank_big (300 keys >= 255, three
                                    values: ties across the chunks); the side list filled to bigcap - 1; no key >= 255.
                                    Known from counts_premise().
  test_short_workspace_is_refused   the i32 and the counts entry with their query minus 256 bytes.

Not reached: the n_dev, key_bits and first_pass parameters of radix_argsort_desc (and the branches of k_rs_* that read them).
No entry sets them, so no input can; they stay as they are here.

What these tests found: d3d_internal_argsort_desc_i32 did not compare the workspace with its query.  The query is the larger
of the radix and the sample-sort carve; at 5000 keys the sample sort needs 79616 of the 87296 bytes, so with 87040 the call
sorted instead of refusing (test_short_workspace_is_refused).  The entry now refuses below its query, like d3d_argsort_desc.

Size: 49 cases -- test_boundary_sizes_every_entry 5 (one per entry and key type: 3 x 21 sizes x 4 families and 2 x 6 x 4, 300
sorts), test_oversized_bucket 27 (9 x 3 key types), test_radix_live_passes 3 (22 + 30 + 11 sorts), test_counts_device_size 12,
test_short_workspace_is_refused 2.  Measured on the MI355X: the file in 2.8 s of wall time, 0.9 s of it in the tests (the
slowest case, the i32 entry's boundary sizes, 0.45 s); the largest single sort is 131073 keys."""
import ctypes

import numpy as np
import pytest
import torch

import sort_reference as ref

pytestmark = pytest.mark.gpu

TAIL = 65536
POISON = 0x77
F32, F64 = 0, 1
ERR_WORKSPACE = -3
_vp, _i64, _i32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_size_t


@pytest.fixture(scope="module")
def lib():
    from d3d_amd import _lib
    lib = _lib.load()
    lib.d3d_internal_argsort_desc_radix.restype = ctypes.c_int
    lib.d3d_internal_argsort_desc_radix.argtypes = [_vp, _i64, _i32, _vp, _vp, _sz, _vp]
    lib.d3d_internal_argsort_i32_bytes.restype = _sz
    lib.d3d_internal_argsort_i32_bytes.argtypes = [_i64]
    lib.d3d_internal_argsort_desc_i32.restype = ctypes.c_int
    lib.d3d_internal_argsort_desc_i32.argtypes = [_vp, _i64, _vp, _vp, _sz, _vp]
    lib.d3d_internal_argsort_counts_bytes.restype = _sz
    lib.d3d_internal_argsort_counts_bytes.argtypes = [_i64]
    lib.d3d_internal_argsort_desc_counts_dev.restype = ctypes.c_int
    lib.d3d_internal_argsort_desc_counts_dev.argtypes = [_vp, _i64, _vp, _i64, _vp, _vp, _sz, _vp]
    return lib


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Call:
    """one entry on one key array: the query's bytes and a 0xA5 tail behind them, a poisoned order"""

    def __init__(self, lib, entry, keys, n_dev=None, max_key_sum=None, short=0):
        self.n = n = len(keys)
        self.keys = T(keys)
        if entry in ("public", "radix"):
            code = {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[keys.dtype]
            self.query = int(lib.d3d_argsort_desc_workspace_bytes(n, code))       # (>= the radix carve, which it contains)
            order_dtype = torch.int64
        else:
            assert keys.dtype == np.int32
            self.query = int((lib.d3d_internal_argsort_i32_bytes if entry == "i32" else lib.d3d_internal_argsort_counts_bytes)(n))
            order_dtype = torch.int32
        assert self.query > 0 and self.query % 256 == 0
        self.ws = torch.full((self.query + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
        self.order = torch.empty(n, dtype=order_dtype, device="cuda")
        self.order.view(torch.uint8).fill_(POISON)
        given = self.query - short
        k, o, w = self.keys.data_ptr(), self.order.data_ptr(), self.ws.data_ptr()
        if entry == "public":
            self.rc = lib.d3d_argsort_desc(k, n, code, o, w, given, None)
        elif entry == "radix":
            self.rc = lib.d3d_internal_argsort_desc_radix(k, n, code, o, w, given, None)
        elif entry == "i32":
            self.rc = lib.d3d_internal_argsort_desc_i32(k, n, o, w, given, None)
        else:
            self.n_dev = None if n_dev is None else T(np.array([n_dev], np.int64))
            self.rc = lib.d3d_internal_argsort_desc_counts_dev(k, n, None if n_dev is None else self.n_dev.data_ptr(), max_key_sum, o, w,
                                                               given, None)
        torch.cuda.synchronize()
        self.tail_clean = bool((self.ws[self.query:] == 0xA5).all())
        self.got = self.order.cpu().numpy()

    def order_poisoned(self):
        return bool((self.order.view(torch.uint8) == POISON).all())


def _check(lib, entry, keys, what):
    c = Call(lib, entry, keys)
    assert c.rc == 0, (what, c.rc)
    assert c.tail_clean, "%s wrote behind the %d bytes of its query" % (what, c.query)
    exp = ref.expected_order(keys)
    assert np.array_equal(c.got, exp), (what, "%d of %d entries differ" % (int(np.sum(c.got != exp)), len(exp)))


ENTRIES = {"public_f32": ("public", np.float32, ref.BOUNDARY_SIZES), "public_f64": ("public", np.float64, ref.BOUNDARY_SIZES),
           "i32": ("i32", np.int32, ref.BOUNDARY_SIZES),
           "radix_f32": ("radix", np.float32, ref.RADIX_SIZES), "radix_f64": ("radix", np.float64, ref.RADIX_SIZES)}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_boundary_sizes_every_entry(lib, name):
    entry, dtype, sizes = ENTRIES[name]
    for n in sizes:
        for family in ref.FAMILIES:
            keys = ref.family_keys(family, dtype, n, np.random.default_rng(n))
            if family == "mixed" and n > 64:                                    # the specials are all there
                if dtype == np.int32:
                    assert {ref.INT_MIN, ref.INT_MAX, -1, 0} <= set(keys.tolist()) and (keys < 0).sum() > n // 4
                else:
                    assert np.isnan(keys).any() and np.isinf(keys).any() and (keys < 0).sum() > n // 4
                    assert np.signbit(keys[keys == 0]).any() and not np.signbit(keys[keys == 0]).all()
                assert len(np.unique(keys)) < 0.9 * n
            _check(lib, entry, keys, (name, n, family))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
@pytest.mark.parametrize("case", [c[0] for c in ref.OVERSIZED])
def test_oversized_bucket(lib, case, dtype):
    keys = ref.oversized_premise(case, dtype)                                   # asserts the bucket sizes the case is there for
    _check(lib, "i32" if dtype == np.int32 else "public", keys, (case, np.dtype(dtype).name))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int32])
def test_radix_live_passes(lib, dtype):
    nb = np.dtype(dtype).itemsize
    entry, sizes = ("i32", (ref.LIVE_SIZE_I32,)) if dtype == np.int32 else ("radix", ref.LIVE_SIZES)
    for n in sizes:
        assert entry == "radix" or n > ref.SS_MAX_N                             # (the i32 entry's radix route)
        for k, live in enumerate(ref.live_sets(dtype)):
            keys = ref.keys_with_live_bytes(dtype, live, n, np.random.default_rng(100 * k + nb))
            assert ref.live_bytes(keys) == frozenset(live)
            _check(lib, entry, keys, (np.dtype(dtype).name, n, live))
        for shift in (0, 32):
            keys = ref.run_keys(dtype, n, shift, np.random.default_rng(nb))
            uni = ref.wavefront_uniformity(keys)
            assert n % ref.WAVE == 1 and ref.live_bytes(keys) == {0, 1, nb - 1}
            if shift == 0:
                assert all(mixed == 0 for _, mixed in uni)
            else:
                assert all(uni[p][1] > 0.9 * (n // ref.WAVE) and uni[p][0] >= 1 for p in (0, 1, nb - 1))
            _check(lib, entry, keys, (np.dtype(dtype).name, n, "runs", shift))


@pytest.mark.parametrize("name", sorted(ref.COUNTS))
def test_counts_device_size(lib, name):
    keys, n_dev, max_key_sum, valid = ref.counts_premise(name)
    c = Call(lib, "counts", keys, n_dev=n_dev, max_key_sum=max_key_sum)
    assert c.rc == 0, c.rc
    assert c.tail_clean, "%s wrote behind the %d bytes of its query" % (name, c.query)
    exp = ref.expected_order(keys[:valid])
    assert np.array_equal(c.got[:valid], exp), (name, "%d of %d entries differ" % (int(np.sum(c.got[:valid] != exp)), valid))


@pytest.mark.parametrize("entry", ["i32", "counts"])
def test_short_workspace_is_refused(lib, entry):
    n = 5000
    if entry == "i32":
        c = Call(lib, entry, ref.family_keys("mixed", np.int32, n, np.random.default_rng(n)), short=256)
    else:
        keys, n_dev, max_key_sum, _ = ref.counts_premise("dev5000")
        c = Call(lib, entry, keys, n_dev=n_dev, max_key_sum=max_key_sum, short=256)
    assert c.rc == ERR_WORKSPACE, c.rc
    assert c.order_poisoned(), "order written by a refused call"
    assert c.tail_clean
