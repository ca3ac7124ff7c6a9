"""Model of the stable descending argsort (d3d_amd/csrc/sort.hip, lds_sort.hpp), numpy only.

expected_order() is the specification, on VALUES: torch's descending stable order (nms.cpp:103) -- NaN first, every NaN equal,
-0 == +0, ties in ascending index; plain stable descending for int32.  Everything else here mirrors how sort.hip ROUTES keys --
the image KeyBits<K>::desc sorts by, the sample rule of k_ss_splitters, the bytes the radix plan looks at, the classes of the
counting sort -- and serves only to state what a crafted input reaches (which bucket overflows, which passes are live): the GPU
tests cannot observe that, so they assert it here before they launch.  No expected order is ever computed from an image.

tests/test_sort_reference.py holds expected_order against torch.sort on the CPU, the images against expected_order, the
premises of every case below, and the constants against the source (a change of the sample rule must change this file too)."""
import numpy as np

# ---------------------------------------------------------------- sort.hip's constants (drift guard: test_sort_reference.py)
SS_SAMPLES = 1024                       # kSsSamples
SS_BUCKET_CAP = 2048                    # kSsBucketCap: the largest bucket sorted in LDS, and the largest one-workgroup sort
SS_MIN_N = 2049                         # kSsMinN
SS_MAX_BUCKETS = 512                    # kSsMaxBuckets
SS_MAX_N = SS_MAX_BUCKETS * 256         # kSsMaxN
SS_KEYS_PER_BUCKET = 192                # ss_buckets: B = clamp(n / 192, 16, kSsMaxBuckets)
SS_MIN_BUCKETS = 16
SS_HASH_MUL = (0x7FEB352D, 0x846CA68B)  # ss_hash: x ^= x >> 16; x *= M0; x ^= x >> 15; x *= M1; x ^= x >> 16
SS_HASH_SHIFT = (16, 15, 16)
RS_TILE = 4096                          # kRsTile: keys per workgroup of the radix and the counting sort
CS_TOP = 255                            # cs_digit: the class "255 or more" leaves through the side list
CS_CHUNK = 256                          # k_cs_rank_big: candidates per round, entries per workgroup
WAVE = 64

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------- the specification
def expected_order(keys):
    """the permutation every entry must return, entry by entry"""
    keys = np.asarray(keys)
    idx = np.arange(len(keys))
    if keys.dtype.kind == "f":
        nan = np.isnan(keys)
        val = np.where(nan, 0, keys)
        return np.lexsort((idx, -val, ~nan))
    assert keys.dtype == np.int32
    return np.lexsort((idx, -keys.astype(np.int64)))


# ---------------------------------------------------------------- KeyBits<K>::desc
def desc_image(keys):
    """the unsigned integer whose ASCENDING order the kernels sort by (premises only)"""
    keys = np.ascontiguousarray(keys)
    if keys.dtype == np.int32:
        return ~(keys.view(np.uint32) ^ np.uint32(0x80000000))
    u = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}[keys.dtype]
    sign = u(1) << u(8 * keys.itemsize - 1)
    b = keys.view(u).copy()
    b[b == sign] = 0                                            # -0 -> +0
    asc = np.where(b & sign != 0, ~b, b | sign)
    img = ~asc
    img[np.isnan(keys)] = 0                                     # NaN: first
    return img.astype(u)


def _keys_of_image(img, dtype):
    """the inverse of desc_image where it is a bijection (no NaN, no zero)"""
    dtype = np.dtype(dtype)
    if dtype == np.int32:
        return ((~img) ^ np.uint32(0x80000000)).view(np.int32)
    u = img.dtype.type
    sign = u(1) << u(8 * dtype.itemsize - 1)
    asc = ~img
    return np.where(asc & sign != 0, asc & ~sign, ~asc).astype(u).view(dtype)


def _image_bytes(keys):
    img = desc_image(keys)
    return img.view(np.uint8).reshape(len(img), img.itemsize)   # column p = the digit of pass p (little endian)


def live_bytes(keys):
    """the passes k_rs_plan keeps: byte positions of the image that are not the same in every key"""
    by = _image_bytes(keys)
    return frozenset(int(p) for p in range(by.shape[1]) if by[:, p].min() != by[:, p].max())


def wavefront_uniformity(keys):
    """per byte position: (wavefronts of k_rs_hist whose keys share the digit, wavefronts that hold two or more digits).
    A wavefront of k_rs_hist is 64 consecutive keys from a multiple of 64 (block and stride are multiples of 64)."""
    by = _image_bytes(keys)
    n = len(by)
    res = []
    for p in range(by.shape[1]):
        uni = sum(1 for s in range(0, n, WAVE) if by[s:s + WAVE, p].min() == by[s:s + WAVE, p].max())
        res.append((uni, (n + WAVE - 1) // WAVE - uni))
    return res


# ---------------------------------------------------------------- k_ss_splitters
def ss_hash(x):
    x = np.asarray(x, np.uint64) & _M32
    x ^= x >> np.uint64(SS_HASH_SHIFT[0])
    x = (x * np.uint64(SS_HASH_MUL[0])) & _M32
    x ^= x >> np.uint64(SS_HASH_SHIFT[1])
    x = (x * np.uint64(SS_HASH_MUL[1])) & _M32
    x ^= x >> np.uint64(SS_HASH_SHIFT[2])
    return x


def sample_positions(n):
    """one sample per stratum of n // 1024 keys, jittered; whatever lies behind 1024 strata is never sampled"""
    assert SS_MIN_N <= n <= SS_MAX_N
    length = np.uint64(n // SS_SAMPLES)
    j = np.arange(SS_SAMPLES, dtype=np.uint64)
    return (j * length + ss_hash(j) % length).astype(np.int64)


def buckets(n):
    return int(min(max(n // SS_KEYS_PER_BUCKET, SS_MIN_BUCKETS), SS_MAX_BUCKETS))


def bucket_sizes(keys):
    """entries per bucket of the sample sort: bucket = number of splitters <= the key's composite (image, index)"""
    n = len(keys)
    idx = np.arange(n)
    rank = np.empty(n, np.int64)
    rank[np.lexsort((idx, desc_image(keys)))] = idx              # composites are unique: their rank stands for them
    nb = buckets(n)
    samples = np.sort(rank[sample_positions(n)])
    splitters = samples[[b * SS_SAMPLES // nb for b in range(1, nb)]]
    return np.bincount(np.searchsorted(splitters, rank, side="right"), minlength=nb)


# ---------------------------------------------------------------- inputs of the boundary tests
FAMILIES = ("mixed", "constant", "two", "ascending")


def family_keys(family, dtype, n, rng):
    dtype = np.dtype(dtype)
    integer = dtype == np.int32
    if family == "constant":
        return np.full(n, -7 if integer else 0.25, dtype)
    if family == "two":
        return rng.integers(0, 2, n).astype(dtype) * 3 - 1
    if family == "ascending":
        return (np.arange(n) - n // 2).astype(dtype)
    if integer:
        s = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int32)
        special = [INT_MIN, INT_MAX, -1, 0, INT_MIN, INT_MAX]
    else:
        s = rng.normal(0, 100, n).astype(dtype)                 # negatives: half of them
        special = [np.nan, 0.0, -0.0, np.inf, -np.inf, np.nan, -0.0, 0.0]
    if n >= 5:
        s[rng.integers(0, n, n // 5)] = s[rng.integers(0, n, n // 5)]        # a fifth tied
    at = rng.choice(n, min(n, len(special)), replace=False)     # (n = 1: NaN / INT_MIN alone, n = 2: two of them)
    s[at] = special[:len(at)]
    return s


# ---------------------------------------------------------------- oversized buckets
def oversized_keys(n, kind, dtype, rng, nans=0):
    """The 1024 sampled positions hold keys of a middle band, so every splitter lies in the band; every other position holds one
    of three values below the band ("tail": they all sort behind the last splitter, into the last bucket), above it ("head":
    the first bucket) or either ("both").  Inside a pile there are three distinct keys: the index decides.
    nans: that many of the keys above the band become NaN (floats; they sort before everything, so they stay in the pile)."""
    dtype = np.dtype(dtype)
    if dtype == np.int32:
        band = rng.integers(-1000, 1001, n).astype(np.int32)
        below, above = np.array([INT_MIN, -5000, -4999], np.int32), np.array([4999, 5000, INT_MAX], np.int32)
    else:
        band = (rng.random(n) * 2 - 1).astype(dtype)
        below, above = np.array([-np.inf, -3.5, -2.0], dtype), np.array([2.0, 3.5, np.inf], dtype)
    sampled = np.zeros(n, bool)
    sampled[sample_positions(n)] = True
    high = {"tail": np.zeros(n, bool), "head": np.ones(n, bool), "both": rng.random(n) < 0.5}[kind]
    pick = rng.integers(0, 3, n)
    keys = np.where(sampled, band, np.where(high, above[pick], below[pick])).astype(dtype)
    if nans:
        assert dtype.kind == "f"
        at = np.flatnonzero(~sampled & high)
        keys[rng.choice(at, nans, replace=False)] = np.nan
    return keys


# (name, n, kind, what the largest buckets must be: "lds2" = 1025 .. 2048, sort_lds<2> inside k_ss_bucket; "fallback" = above
# the cap, ranked from global memory; exact sizes where the arithmetic fixes them: the pile of n - 1024 unsampled keys plus the
# 64 samples behind the last / before the first of 15 splitters)
OVERSIZED = (
    ("tail_3008", 3008, "tail", "lds2", 2048),
    ("head_3008", 3008, "head", "lds2", 2048),
    ("tail_3009", 3009, "tail", "fallback", 2049),
    ("head_3009", 3009, "head", "fallback", 2049),
    ("tail_3072", 3072, "tail", "fallback", 2112),
    ("head_3072", 3072, "head", "fallback", 2112),
    ("both_4096", 4096, "both", "lds2", None),
    ("both_8192", 8192, "both", "fallback", None),
    ("tail_16384", 16384, "tail", "fallback", None),
)


def oversized_case(name, dtype):
    """-> keys, the pile's bucket sizes (two for "both"), the largest of the other buckets -- the same keys on every call"""
    at = [c[0] for c in OVERSIZED].index(name)
    _, n, kind, _, _ = OVERSIZED[at]
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(1000 * at + dtype.itemsize + (dtype.kind == "i"))
    nans = 5 if dtype.kind == "f" and kind in ("head", "both") else 0
    keys = oversized_keys(n, kind, dtype, rng, nans)
    sizes = np.sort(bucket_sizes(keys))[::-1]
    return keys, sizes[:2 if kind == "both" else 1], sizes[2 if kind == "both" else 1]


def oversized_premise(name, dtype):
    """asserts what the case is there to reach; returns its keys"""
    _, n, kind, reach, exact = OVERSIZED[[c[0] for c in OVERSIZED].index(name)]
    keys, largest, next_largest = oversized_case(name, dtype)
    for m in largest:
        if reach == "lds2":
            assert SS_BUCKET_CAP // 2 < m <= SS_BUCKET_CAP, (name, largest)
        else:
            assert m > SS_BUCKET_CAP, (name, largest)
        assert exact is None or m == exact, (name, largest)
    assert next_largest <= SS_BUCKET_CAP // 2, (name, next_largest)     # every other bucket: sort_lds<1>
    return keys


# ---------------------------------------------------------------- radix plan: which passes are live
_TOP_OK = np.array([t for t in range(256) if t not in (0x00, 0x7F, 0x80, 0xFF)], np.uint8)


def keys_with_live_bytes(dtype, live, n, rng):
    """keys whose image varies in exactly the byte positions `live` (0 = lowest).  Floats: the image's top byte (sign and the
    exponent's high seven bits) never takes 0x00 / 0xFF (exponent all ones: inf, NaN) nor 0x7F / 0x80 (exponent zero: +-0,
    subnormals), whatever the lower bytes are -- finite, normal, never zero, so the image is a bijection of the bits."""
    dtype = np.dtype(dtype)
    nb = dtype.itemsize
    live = frozenset(live)
    assert all(0 <= p < nb for p in live) and (n >= 2 or not live)
    by = np.empty((n, nb), np.uint8)
    for p in range(nb):
        allowed = _TOP_OK if p == nb - 1 and dtype.kind == "f" else np.arange(256, dtype=np.uint8)
        if p in live:
            by[:, p] = rng.choice(allowed, n)
            by[:2, p] = rng.choice(allowed, 2, replace=False)    # (varies whatever the draw)
        else:
            by[:, p] = rng.choice(allowed)
    img = np.ascontiguousarray(by).view(np.uint32 if nb == 4 else np.uint64).ravel()
    return _keys_of_image(img, dtype)


def live_sets(dtype):
    """each single pass, {0, top}, {1, 2}, the lowest three, all, none"""
    nb = np.dtype(dtype).itemsize
    return [(p,) for p in range(nb)] + [(0, nb - 1), (1, 2), (0, 1, 2), tuple(range(nb)), ()]


def run_keys(dtype, n, shift, rng):
    """keys constant over runs of 64 that start at 64 k - shift: with shift = 0 every wavefront of k_rs_hist is uniform in every
    pass, with shift = 32 every full wavefront holds two keys.  Bytes 0, 1 and the top byte vary between runs."""
    nb = np.dtype(dtype).itemsize
    vals = keys_with_live_bytes(dtype, (0, 1, nb - 1), n // WAVE + 2, rng)
    return vals[(np.arange(n) + shift) // WAVE]


# ---------------------------------------------------------------- the counting sort's contract
def counts_case(n, n_dev, rng, planted=(), fill=True, tight=False):
    """-> keys int32 [n], max_key_sum.  keys[:n_dev] >= 0 with sum <= max_key_sum <= n: `planted` at random places, the rest
    0 (or, with fill, small counts and a few up to 254 as far as the sum allows: ties everywhere).  keys[n_dev:] are garbage
    (INT_MAX, INT_MIN, -1) that the entry must not read into the result.  tight: max_key_sum = the sum, else n."""
    head = np.zeros(n_dev, np.int64)
    at = rng.choice(n_dev, len(planted), replace=False) if len(planted) else np.zeros(0, np.int64)
    head[at] = planted
    budget = n - int(head.sum())
    assert budget >= 0
    if fill and n_dev > len(planted):
        rest = rng.permutation(np.setdiff1d(np.arange(n_dev), at))
        draw = np.where(rng.random(len(rest)) < 0.004, rng.integers(100, 255, len(rest)), rng.integers(0, 3, len(rest)))
        head[rest] = np.where(np.cumsum(draw) <= budget, draw, 0)
    keys = np.empty(n, np.int32)
    keys[:n_dev] = head
    keys[n_dev:] = np.resize(np.array([INT_MAX, INT_MIN, -1], np.int32), n - n_dev)
    return keys, (int(head.sum()) if tight else n)


# name: (n, n_dev or None = no device-side size, planted, fill, tight, keys >= 255)
COUNTS = {
    "n1_dev0": (1, 0, (), False, False, 0),
    "n1_dev1": (1, 1, (1,), False, False, 0),
    "dev0": (5000, 0, (), False, False, 0),
    "dev1": (5000, 1, (256,), False, False, 1),
    "dev4095": (5000, 4095, (253, 254, 255, 255, 256, 257, 257), True, False, 5),
    "dev4096": (5000, 4096, (253, 254, 255, 255, 256, 257, 257), True, False, 5),
    "dev4097": (5000, 4097, (253, 254, 255, 255, 256, 257, 257), True, False, 5),
    "dev5000": (5000, 5000, (253, 254, 255, 255, 256, 257, 257), True, False, 5),
    "null": (5000, None, (253, 254, 255, 255, 256, 257, 257), True, False, 5),
    "second_chunk": (100000, 4200, (255,) * 100 + (256,) * 100 + (257,) * 100 + (253, 254) * 20, True, False, 300),
    "tight": (5000, 19, (255,) * 19, False, True, 19),
    "no_big": (5000, 4500, (254, 254, 253), True, False, 0),
}


def counts_named(name):
    """-> keys, n_dev (None: NULL), max_key_sum, the number of valid keys -- the same on every call"""
    n, n_dev, planted, fill, tight, _ = COUNTS[name]
    rng = np.random.default_rng(sorted(COUNTS).index(name))
    valid = n if n_dev is None else n_dev
    keys, mks = counts_case(n, valid, rng, planted, fill, tight)
    return keys, n_dev, mks, valid


def counts_premise(name):
    keys, n_dev, mks, valid = counts_named(name)
    n, big = COUNTS[name][0], COUNTS[name][5]
    head = keys[:valid].astype(np.int64)
    assert len(keys) == n and (head >= 0).all() and head.sum() <= mks <= n, name
    assert int((head >= CS_TOP).sum()) == big, name
    assert big <= mks // CS_TOP + 1, name                       # the side list (counts_bigcap) holds them
    if valid < n:
        assert set(keys[valid:].tolist()) <= {INT_MAX, INT_MIN, -1}
    return keys, n_dev, mks, valid


# ---------------------------------------------------------------- sizes of tests/test_gpu_sort.py
BOUNDARY_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3265, 4096, 5000, 98303, 98304, 131071, 131072,
                  131073)
RADIX_SIZES = (1, 64, 4095, 4096, 4097, 8193)
LIVE_SIZES = (4097, 8193)               # the radix-only entry (fp32, fp64)
LIVE_SIZE_I32 = 131073                  # the i32 entry's only way to its radix route
