"""The Python front of the sharded voxelizer (d3d_amd/voxel/sharded.py) on the CPU: the NumPy twins of the kernels behind a
recorder.  What a communicator and a caller's `ops` see of a call -- which collectives and compute steps, in which order, with
how many arguments and which keywords -- is the contract of INTEGRATION.md section 6; it is pinned here call by call, with the
result's keys and `last_stats`, the lock-step repeat after a status overflow, the first-index tail of the bitmap exchange, and
every refusal word for word."""
import numpy as np
import pytest
import torch

from d3d_amd import _lib
from d3d_amd.voxel import sharded
from d3d_amd.voxel.sharded import LocalComm, ShardedVoxelGenerator
from sharded_helpers import NumpyOps
from test_sharded import BOUNDS, SHAPE, _check, _check_owned, _cloud

TABLE_FULL = "voxelize_3d_reduce: internal hash table overflow"


class Recorder:
    """`inner` (a comm or an ops) with every method call logged as "who.method/positional arguments/keywords"; hooks[method]
    (if any) sees the method's result before the caller does"""

    def __init__(self, who, inner, log, hooks=None):
        self._who, self._inner, self._log, self._hooks = who, inner, log, hooks or {}

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def call(*a, **k):
            self._log.append("%s.%s/%d/%s" % (self._who, name, len(a), ",".join(sorted(k))))
            out = attr(*a, **k)
            return self._hooks[name](out) if name in self._hooks else out
        return call


def _recorded(ops=None, hooks=None, **kw):
    log = []
    gen = ShardedVoxelGenerator(BOUNDS, SHAPE, comm=Recorder("comm", LocalComm(), log),
                                ops=Recorder("ops", ops or NumpyOps(), log, hooks), **kw)
    return gen, log


@pytest.fixture(scope="module")
def cloud():
    return _cloud(500, 1)


# ---- 1. the call sequence, the result's keys and last_stats of every exchange ----
_LOCAL = "ops.voxelize_reduce/5/max_points,want_coords"
_OWNER_HEAD = [_LOCAL, "ops.owner_pack/11/points_in_shard", "comm.exchange_counts/1/", "comm.all_to_all/3/"]
_OWNER_NUMBER = ["ops.owner_mark_first/3/", "comm.all_reduce/2/", "ops.owner_number/4/", "ops.owner_reply/2/", "comm.all_to_all/3/",
                 "ops.owner_map/3/"]
_OWNER_ROWS = ["comm.all_to_all/3/", "ops.owner_dense/4/"]
_OWNER_GATHER = ["comm.all_gather_int/2/", "comm.all_gather_var/2/", "comm.all_gather_var/2/", "ops.owner_replicate/5/sizes"]
_MERGE = "ops.owner_merge/6/flags,point_off"
_LEGACY_TAIL = ["ops.compact_keys/2/", "ops.build_table_owned/9/", "comm.all_reduce/2/", "ops.finalize_owned/7/", "ops.compose_map/4/"]
_GRID = ["coords", "voxel_npoints", "aggregates", "points_mapping"]
_OWNER_STATS = dict(exchange="owner", numbering="first-point bitmap", voxels=441, owned_voxels=441, ranks=1, all_to_all_bytes_sent=0,
                    all_to_all_bytes_received=0, reply_bytes_sent=0, all_reduce_bytes=64)
_BITMAP = dict(
    log=["comm.all_gather_int/2/", "ops.voxelize_reduce/5/", "ops.bitmap_mark/3/", "comm.all_gather_var/2/",
         "ops.compact_from_bitmaps/3/rank"] + _LEGACY_TAIL,
    keys=_GRID,
    stats=dict(exchange="bitmap", numbering="ownership", voxels=441, ranks=1, all_gather_bytes_per_rank=4408, all_reduce_bytes=10584))
_KEYS = dict(
    log=["comm.all_gather_int/2/", "ops.voxelize_reduce/5/", "comm.all_gather_var/2/", "ops.compact_index/2/status_stride",
         "ops.compact_keys/2/", "ops.build_table/10/want_keys", "comm.all_reduce/2/", "comm.all_reduce/2/", "ops.finalize/9/",
         "ops.compose_map/4/"],
    keys=_GRID,
    stats=dict(exchange="keys", numbering="first-index", voxels=441, ranks=1, all_gather_bytes_per_rank=4008, all_reduce_bytes=12348))
CASES = {
    "owner": dict(
        kw=dict(exchange="owner"), log=_OWNER_HEAD + [_MERGE] + _OWNER_NUMBER + _OWNER_GATHER, keys=_GRID,
        stats=dict(_OWNER_STATS, all_gather_bytes_per_rank=441 * 52)),
    "owner, owned voxels": dict(
        kw=dict(exchange="owner", replicate=False), log=_OWNER_HEAD + [_MERGE] + _OWNER_NUMBER,
        keys=["coords", "voxel_npoints", "aggregates", "voxel_ids", "points_mapping", "num_voxels"],
        stats=dict(_OWNER_STATS, all_gather_bytes_per_rank=0)),
    "owner, owned voxels, dense": dict(
        kw=dict(exchange="owner", replicate=False, max_points=3), log=_OWNER_HEAD + [_MERGE] + _OWNER_ROWS + _OWNER_NUMBER,
        keys=["coords", "voxel_npoints", "aggregates", "voxel_ids", "points_mapping", "num_voxels", "voxels", "voxel_pmask"],
        stats=dict(_OWNER_STATS, all_gather_bytes_per_rank=0, rows_all_to_all_bytes_sent=0)),
    "owner, dense": dict(
        kw=dict(exchange="owner", max_points=3),
        log=_OWNER_HEAD + [_MERGE] + _OWNER_ROWS + _OWNER_NUMBER + _OWNER_GATHER + ["comm.all_gather_var/2/", "comm.all_gather_var/2/"],
        keys=_GRID + ["voxels", "voxel_pmask"],
        stats=dict(_OWNER_STATS, all_gather_bytes_per_rank=441 * 52, rows_all_to_all_bytes_sent=0)),
    "keys": dict(_KEYS, kw=dict(exchange="keys")),
    "bitmap": dict(_BITMAP, kw=dict(exchange="bitmap")),
    "auto": dict(_KEYS, kw=dict(exchange="auto")),        # (a key list of 501 words is shorter than the grid's bitmap of 551)
}


@pytest.mark.parametrize("case", list(CASES))
def test_call_sequence_result_keys_and_stats(case, cloud):
    want = CASES[case]
    gen, log = _recorded(**want["kw"])
    res = gen(torch.from_numpy(cloud))
    assert log == want["log"]
    assert list(res.keys()) == want["keys"]
    assert gen.last_stats == want["stats"]


# ---- 2. the lock-step repeat of the owner-computes exchange ----
def _raise_status_once(bits, word):
    """a hook for owner_pack: `bits` appear in the status word of the first call's count vector"""
    seen = []

    def hook(out):
        if not seen:
            seen.append(1)
            out[4][word] |= bits
        return out
    return hook


@pytest.mark.parametrize("max_points", [0, 3])
def test_owner_status_overflow_repeats_every_step_in_lock_step(max_points, cloud):
    first = CASES["owner, owned voxels, dense" if max_points else "owner, owned voxels"]["log"]
    gen, log = _recorded(hooks={"owner_pack": _raise_status_once(_lib.STATUS_PACK_OVERFLOW, LocalComm.world)}, exchange="owner",
                         replicate=False, max_points=max_points or None)
    res = gen(torch.from_numpy(cloud))
    assert log == first[:3] + ["ops.voxelize_reduce/5/max_points,plain,want_coords"] + first[1:]
    _check_owned(res, cloud, slice(0, len(cloud)), "mean", max_points=max_points)


def test_owner_table_overflow_is_an_error(cloud):
    gen, log = _recorded(hooks={"owner_pack": _raise_status_once(_lib.STATUS_TABLE_FULL, LocalComm.world)}, exchange="owner")
    with pytest.raises(RuntimeError) as e:
        gen(torch.from_numpy(cloud))
    assert str(e.value) == TABLE_FULL
    assert log == CASES["owner"]["log"][:3]


# ---- 3. the same rule on the replicated-grid exchanges ----
class _StatusOnce(NumpyOps):
    """compact_index / compact_from_bitmaps report `bits` among the ranks' status bits, once"""

    def __init__(self, bits):
        self._bits = bits

    def _report(self, out):
        bits, self._bits = self._bits, 0
        return out[0], out[1], out[2] | bits

    def compact_index(self, *a, **k):
        return self._report(super().compact_index(*a, **k))

    def compact_from_bitmaps(self, *a, **k):
        return self._report(super().compact_from_bitmaps(*a, **k))


@pytest.mark.parametrize("exchange", ["keys", "bitmap"])
def test_legacy_status_overflow_repeats_once_on_the_general_path(exchange, cloud):
    once = CASES[exchange]["log"]
    gen, log = _recorded(ops=_StatusOnce(_lib.STATUS_BIN_OVERFLOW), exchange=exchange)
    res = gen(torch.from_numpy(cloud))
    stop = 5 if exchange == "bitmap" else 4            # ... through the step that reads the status
    assert log == once[:stop] + [once[0], "ops.voxelize_reduce/5/plain"] + once[2:]
    _check(res, cloud, slice(0, len(cloud)), "mean")


@pytest.mark.parametrize("exchange", ["keys", "bitmap"])
def test_legacy_table_overflow_is_an_error(exchange, cloud):
    gen, _ = _recorded(ops=_StatusOnce(_lib.STATUS_TABLE_FULL), exchange=exchange)
    with pytest.raises(RuntimeError) as e:
        gen(torch.from_numpy(cloud))
    assert str(e.value) == TABLE_FULL


# ---- 4. the bitmap exchange numbered by first indices (more ranks than the ownership bookkeeping holds) ----
@pytest.mark.parametrize("reduction", ["mean", "max"])
def test_bitmap_exchange_first_index_tail(reduction, cloud, monkeypatch):
    monkeypatch.setattr(sharded, "_MAX_OWNER_WORLD", 0)
    gen, log = _recorded(exchange="bitmap", reduction=reduction)
    res = gen(torch.from_numpy(cloud))
    assert gen.last_stats["numbering"] == "first-index" and gen.last_stats["exchange"] == "bitmap"
    assert gen.last_stats["all_reduce_bytes"] == 12348
    reduces = ["comm.all_reduce/2/"] * (2 if reduction == "mean" else 3)          # table (, counts), first indices
    assert log == CASES["bitmap"]["log"][:4] + ["ops.compact_from_bitmaps/3/rank", "ops.compact_keys/2/",
                                               "ops.build_table/10/want_keys"] + reduces + ["ops.finalize/9/", "ops.compose_map/4/"]
    _check(res, cloud, slice(0, len(cloud)), reduction)


# ---- 5. refusals, word for word, the first that applies ----
class _OldComm:
    """the replicated-grid protocol only: no exchange_counts, no all_to_all"""
    rank, world = 0, 1

    def all_gather_int(self, v, dev):
        return [int(v)]

    def all_gather_var(self, t, sizes):
        return t

    def all_reduce(self, t, op):
        return t


_NO_OWNER = ("comm lacks exchange_counts / all_to_all: replicate=False and max_points need the owner-computes exchange "
             "(INTEGRATION.md section 6)")
REFUSALS = [
    (dict(reduction="median", shape=[88, 100], exchange="rows"), ValueError, "Unsupported reduction type in VoxelGenerator!"),
    (dict(reduction=None), ValueError, "Unsupported reduction type in VoxelGenerator!"),
    (dict(bounds=BOUNDS[:5], exchange="rows"), ValueError, "bounds must have 6 entries and shape 3 positive entries"),
    (dict(shape=[88, 100], replicate=False, exchange="keys"), ValueError, "bounds must have 6 entries and shape 3 positive entries"),
    (dict(shape=[88, 0, 4]), ValueError, "bounds must have 6 entries and shape 3 positive entries"),
    (dict(exchange="rows", comm=_OldComm(), replicate=False), ValueError, "exchange must be owner, auto, keys or bitmap"),
    (dict(comm=_OldComm(), replicate=False, resident=True), TypeError, _NO_OWNER),
    (dict(comm=_OldComm(), max_points=300), TypeError, _NO_OWNER),
    (dict(exchange="keys", replicate=False, resident=True, max_points=300), ValueError, "replicate=False needs exchange='owner'"),
    (dict(exchange="bitmap", resident=True, max_points=300), ValueError,
     "resident needs the dense contract (max_points) with replicate=False"),
    (dict(replicate=False, resident=True), ValueError, "resident needs the dense contract (max_points) with replicate=False"),
    (dict(exchange="auto", max_points=300), ValueError, "max_points (the dense contract) needs exchange='owner'"),
    (dict(max_points=257, replicate=False), ValueError, "max_points <= 256 on the sharded path"),
]


@pytest.mark.parametrize("kw,error,text", REFUSALS)
def test_constructor_refusals(kw, error, text):
    kw = dict(dict(bounds=BOUNDS, shape=SHAPE, comm=LocalComm(), ops=NumpyOps()), **kw)
    with pytest.raises(error) as e:
        ShardedVoxelGenerator(**kw)
    assert str(e.value) == text


def test_dense_contract_refuses_points_of_another_width(cloud):
    gen, log = _recorded(exchange="owner", max_points=3)
    wide = np.concatenate([cloud, cloud[:, :1]], 1)
    with pytest.raises(ValueError) as e:
        gen(torch.from_numpy(wide))
    assert str(e.value) == "the sharded dense contract needs points[n, 4]" and log == []
