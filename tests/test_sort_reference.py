"""The model of the argsort kernels (tests/sort_reference.py) without a GPU: its order against torch's stable descending sort
on the CPU (the specification, nms.cpp:103), its mirror of KeyBits<K>::desc against that order, the premises of every crafted
case of tests/test_gpu_sort.py (which bucket overflows, which radix passes are live, the counting sort's contract), and its
constants against d3d_amd/csrc/sort.hip."""
import os
import re

import numpy as np
import pytest
import torch

import sort_reference as ref

DTYPES = [np.float32, np.float64, np.int32]
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "d3d_amd", "csrc")


def _spec_inputs(dtype):
    """every family at sizes with and without room for ties, and the special values side by side"""
    for n in (1, 2, 7, 64, 1000, 5000):
        for family in ref.FAMILIES:
            yield "%s_%d" % (family, n), ref.family_keys(family, dtype, n, np.random.default_rng(n))
    if np.dtype(dtype).kind == "f":
        yield "specials", np.array([0.0, np.nan, -0.0, np.inf, 1.0, -np.inf, -0.0, np.nan, 0.0, 1.0, -1.0, np.inf, -np.nan,
                                    np.finfo(dtype).tiny / 4, -np.finfo(dtype).tiny / 4, np.finfo(dtype).max], dtype)
    else:
        yield "specials", np.array([0, ref.INT_MIN, -1, ref.INT_MAX, 0, ref.INT_MIN, 1, ref.INT_MAX, -1], np.int32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_expected_order_is_torchs_stable_descending_sort(dtype):
    for name, keys in _spec_inputs(dtype):
        want = torch.sort(torch.from_numpy(keys), descending=True, stable=True).indices.numpy()
        assert np.array_equal(ref.expected_order(keys), want), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_order_is_the_expected_order(dtype):
    for name, keys in _spec_inputs(dtype):
        by_image = np.lexsort((np.arange(len(keys)), ref.desc_image(keys)))
        assert np.array_equal(by_image, ref.expected_order(keys)), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_image_inverse(dtype):
    keys = ref.keys_with_live_bytes(dtype, range(np.dtype(dtype).itemsize), 4097, np.random.default_rng(1))
    assert np.array_equal(ref._keys_of_image(ref.desc_image(keys), dtype).view(np.uint8), keys.view(np.uint8))


def test_sample_positions():
    sizes = [n for n in ref.BOUNDARY_SIZES if ref.SS_MIN_N <= n <= ref.SS_MAX_N] + [c[1] for c in ref.OVERSIZED]
    assert ref.SS_MIN_N in sizes and ref.SS_MAX_N in sizes
    for n in sizes:
        pos = ref.sample_positions(n)
        assert len(pos) == ref.SS_SAMPLES == len(np.unique(pos)) and pos.min() >= 0 and pos.max() < n, n
        assert (pos // (n // ref.SS_SAMPLES) == np.arange(ref.SS_SAMPLES)).all(), n          # one per stratum
    assert ref.sample_positions(131071).max() < 131071 - 1023                                # the unsampled trailing keys
    assert [ref.buckets(n) for n in (2049, 3008, 3072, 3264, 98303, 98304, 131072)] == [16, 16, 16, 17, 511, 512, 512]
    assert ref.sample_positions(2049).max() < 2048                                           # strata of 2 keys


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [c[0] for c in ref.OVERSIZED])
def test_oversized_premises(name, dtype):
    keys = ref.oversized_premise(name, dtype)
    _, n, kind, _, _ = ref.OVERSIZED[[c[0] for c in ref.OVERSIZED].index(name)]
    assert len(keys) == n <= 16384                      # (the fallback is quadratic in the bucket: one workgroup, milliseconds)
    if np.dtype(dtype).kind == "f" and kind != "tail":
        assert np.isnan(keys).sum() == 5
    sizes = np.sort(ref.bucket_sizes(keys))[::-1]
    if name == "both_4096":
        assert 1500 < sizes[1] <= sizes[0] < 1700       # 1536 +- 40 keys of either pile, 48 / 49 samples
    if name == "tail_16384":
        assert 15360 < sizes[0] < 15380                 # 15360 unsampled keys and the samples behind the last splitter


@pytest.mark.parametrize("dtype", DTYPES)
def test_ordinary_keys_stay_in_one_lds_pass(dtype):
    """at the sizes of the crafted cases, random keys with ties reach neither sort_lds<2> inside a bucket nor the fallback;
    keys in index order do where many trailing keys are never sampled: constant and ascending keys at n = 5000 pile the 904
    keys behind the last stratum into the last (first) bucket, with the 40 (39) strata beyond the outermost splitter"""
    for n in sorted({c[1] for c in ref.OVERSIZED}):
        keys = ref.family_keys("mixed", dtype, n, np.random.default_rng(n))
        assert ref.bucket_sizes(keys).max() <= ref.SS_BUCKET_CAP // 4, n          # (424 at most: far from the 1025 of sort_lds<2>)
    assert ref.bucket_sizes(ref.family_keys("constant", dtype, 5000, None)).max() == 1064
    assert ref.bucket_sizes(ref.family_keys("ascending", dtype, 5000, None)).max() == 1063
    for n in ref.BOUNDARY_SIZES:                        # the boundary test never meets the fallback by accident
        if ref.SS_MIN_N <= n <= ref.SS_MAX_N:
            for family in ref.FAMILIES:
                keys = ref.family_keys(family, dtype, n, np.random.default_rng(n))
                sizes = ref.bucket_sizes(keys)
                assert sizes.sum() == n and sizes.max() <= ref.SS_BUCKET_CAP, (n, family)


@pytest.mark.parametrize("dtype", DTYPES)
def test_live_byte_premises(dtype):
    nb = np.dtype(dtype).itemsize
    sets = ref.live_sets(dtype)
    counts = {len(s) for s in sets}
    assert {0, 1, 2, 3, nb} <= counts                                    # odd and even numbers of live passes, none, all
    assert any(s and max(s) < nb - 1 for s in sets)                      # a last live pass below the top byte
    assert all((p,) in sets for p in range(nb))
    sizes = (ref.LIVE_SIZE_I32,) if dtype == np.int32 else ref.LIVE_SIZES
    for n in sizes:
        for k, live in enumerate(sets):
            keys = ref.keys_with_live_bytes(dtype, live, n, np.random.default_rng(100 * k + nb))
            assert ref.live_bytes(keys) == frozenset(live), (n, live)
            if np.dtype(dtype).kind == "f":
                assert np.isfinite(keys).all() and (np.abs(keys) >= np.finfo(dtype).tiny).all(), (n, live)
            assert len(np.unique(ref.desc_image(keys))) == len(np.unique(keys.view("u%d" % nb)))      # bijection of the bits
        assert n % ref.WAVE != 0 and n > ref.RS_TILE
        waves = (n + ref.WAVE - 1) // ref.WAVE
        aligned = ref.run_keys(dtype, n, 0, np.random.default_rng(nb))
        assert ref.live_bytes(aligned) == {0, 1, nb - 1}
        assert all(u == (waves, 0) for u in ref.wavefront_uniformity(aligned))               # every pass: the one-lane branch
        shifted = ref.wavefront_uniformity(ref.run_keys(dtype, n, 32, np.random.default_rng(nb)))
        for p in range(nb):                             # live passes: two digits in a full wavefront, unless neighbours agree
            if p in (0, 1, nb - 1):                     # (1 in 256, or 1 in 252); the last wavefront is a single key
                assert shifted[p][1] >= waves - 2 - waves // 64 and shifted[p][0] >= 1, (p, shifted[p])
            else:
                assert shifted[p] == (waves, 0)


@pytest.mark.parametrize("name", sorted(ref.COUNTS))
def test_counts_premises(name):
    keys, n_dev, mks, valid = ref.counts_premise(name)
    n = len(keys)
    bigcap = mks // ref.CS_TOP + 1
    big = int((keys[:valid] >= ref.CS_TOP).sum())
    if name == "second_chunk":
        assert big > ref.CS_CHUNK and (n + ref.RS_TILE - 1) // ref.RS_TILE - (valid + ref.RS_TILE - 1) // ref.RS_TILE == 23
        assert len(np.unique(keys[:valid][keys[:valid] >= ref.CS_TOP])) == 3                  # ties across the chunks
    if name == "tight":
        assert big == bigcap - 1 and mks == int(keys[:valid].sum()) and set(keys[:valid].tolist()) == {255}
    if name == "no_big":
        assert big == 0 and keys[:valid].max() == 254
    if valid > 1000:
        assert {253, 254} <= set(keys[:valid].tolist()) and np.bincount(keys[:valid]).max() > valid // 4


def test_counts_cases_cover_the_issue():
    pairs = {(c[0], c[1]) for c in ref.COUNTS.values()}
    assert {(1, 0), (1, 1), (5000, 0), (5000, 1), (5000, 4095), (5000, 4096), (5000, 4097), (5000, 5000), (5000, None)} <= pairs


# ---------------------------------------------------------------- drift guard
def _source(name):
    return open(os.path.join(SRC, name)).read()


def _constant(src, name):
    m = re.search(r"\b%s\s*=\s*(\d+)\b" % name, src)
    assert m, "sort.hip no longer defines %s as a literal: update tests/sort_reference.py" % name
    return int(m.group(1))


def test_model_constants_match_the_source():
    src = _source("sort.hip")
    hint = ": the sample rule of sort.hip changed -- update tests/sort_reference.py (and the cases built on it)"
    for name, mine in (("kSsSamples", ref.SS_SAMPLES), ("kSsBucketCap", ref.SS_BUCKET_CAP), ("kSsMinN", ref.SS_MIN_N),
                       ("kSsMaxBuckets", ref.SS_MAX_BUCKETS)):
        assert _constant(src, name) == mine, name + hint
    assert re.search(r"\bkRsTile\s*=\s*kRsThreads\s*\*\s*kRsItems\b", src), "kRsTile" + hint
    assert _constant(src, "kRsThreads") * _constant(src, "kRsItems") == ref.RS_TILE, "kRsTile" + hint
    m = re.search(r"\bkSsMaxN\s*=\s*\(int64_t\)kSsMaxBuckets\s*\*\s*(\d+)", src)
    assert m and ref.SS_MAX_BUCKETS * int(m.group(1)) == ref.SS_MAX_N, "kSsMaxN" + hint
    body = re.search(r"uint32_t ss_hash\(uint32_t x\)\s*\{(.*?)\}", src, re.S)
    assert body, "ss_hash" + hint
    assert tuple(int(v, 16) for v in re.findall(r"x \*= (0x[0-9a-fA-F]+)u", body.group(1))) == ref.SS_HASH_MUL, "ss_hash" + hint
    assert tuple(int(v) for v in re.findall(r"x \^= x >> (\d+)", body.group(1))) == ref.SS_HASH_SHIFT, "ss_hash" + hint
    m = re.search(r"ss_buckets\(int64_t n\)\s*\{\s*return \(int\)std::min<int64_t>\(std::max<int64_t>\(n / (\d+), (\d+)\), kSsMaxBuckets\)", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (ref.SS_KEYS_PER_BUCKET, ref.SS_MIN_BUCKETS), "ss_buckets" + hint
    for line in ("const uint32_t len = n / kSsSamples;",
                 "const uint32_t pos = (uint32_t)j * len + ss_hash((uint32_t)j) % len;",
                 "const int j = (int)((long long)b * kSsSamples / B);",
                 "if (m > (uint32_t)kSsBucketCap) {",
                 "if (n <= kSsBucketCap && !radix_only) {"):
        assert line in src, repr(line) + hint
    assert "255u - ((uint32_t)c < 255u ? (uint32_t)c : 255u)" in src and ref.CS_TOP == 255, "cs_digit" + hint
    assert "for (uint32_t c0 = 0; c0 < kb; c0 += 256)" in src and ref.CS_CHUNK == 256, "k_cs_rank_big" + hint
    assert _constant(_source("common.hpp"), "kWave") == ref.WAVE
