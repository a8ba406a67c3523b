"""CPU tests of the batched map's host side (no GPU): the batch planner of MRG_FLAG_STREAM
(mrg_run.cpp stream_plan, through mrg_test_stream_plan), the new entry points' behaviour without a
device, and the constants the three bindings share."""
import ctypes as C
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_py(sizes, B):
    """The planner restated: a batch is a maximal run of consecutive files whose sizes sum to at most
    B; a file larger than B is a batch of its own."""
    first, i = [], 0
    while i < len(sizes):
        first.append(i)
        total = sizes[i]
        i += 1
        while i < len(sizes) and total + sizes[i] <= B:
            total += sizes[i]
            i += 1
    return first


def check_plan(sizes, B):
    from mapreduce_rust_amd import native
    first = native.stream_plan(sizes, B)
    assert first == plan_py(sizes, B), (sizes, B)
    # consecutive, every file exactly once, none above B unless it is a single file, and maximal
    assert first == sorted(set(first)) and (first[0] == 0 if sizes else first == [])
    ends = first[1:] + [len(sizes)]
    for a, b in zip(first, ends):
        assert a < b
        total = sum(sizes[a:b])
        assert total <= B or b - a == 1, (sizes, B, a, b)
        if b < len(sizes):
            assert total + sizes[b] > B, (sizes, B, a, b)   # the next file did not fit
    return first


def test_plan_hand_made():
    assert check_plan([], 100) == []
    assert check_plan([0, 0, 0, 0], 100) == [0]
    assert check_plan([0, 0, 0], 0) == [0]
    assert check_plan([500], 100) == [0]
    assert check_plan([10, 500, 10], 100) == [0, 1, 2]
    assert check_plan([0, 500, 0, 0, 10], 100) == [0, 1, 2]          # zero-length files join their neighbours
    assert check_plan([50, 50, 50, 50], 100) == [0, 2]               # sums exactly equal to B
    assert check_plan([100, 100], 100) == [0, 1]
    assert check_plan([60, 40, 1], 100) == [0, 2]
    assert check_plan([1, 1, 0, 2, 0, 1], 1) == [0, 1, 3, 4]          # B = 1
    assert check_plan([3, 0, 3], 1) == [0, 1, 2]
    assert check_plan([1 << 40, 1 << 40, 5], 1 << 30) == [0, 1, 2]
    assert check_plan([(1 << 64) - 1, (1 << 64) - 1], (1 << 64) - 1) == [0, 1]   # no overflow of the sum
    assert check_plan([5, 5, 5], (1 << 64) - 1) == [0]


def test_plan_random():
    rng = random.Random(18)
    for trial in range(200):
        n = rng.randint(0, 40)
        B = rng.choice([1, 2, 7, 100, 1000, 1 << 30])
        sizes = [rng.choice([0, 0, 1, rng.randint(0, B), rng.randint(0, 2 * B), B, B + 1]) for _ in range(n)]
        check_plan(sizes, B)


def test_plan_null_arguments():
    from mapreduce_rust_amd import native
    L = native.load()
    f = L.mrg_test_stream_plan
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_void_p]
    n = C.c_size_t(7)
    assert f(None, 0, 10, None, C.byref(n)) == 0 and n.value == 0
    assert f(None, 3, 10, None, C.byref(n)) == native.EINVAL
    assert f(None, 0, 10, None, None) == native.EINVAL


def test_no_gpu_is_a_clean_error(tmp_path):
    import torch
    from mapreduce_rust_amd import native
    L = native.load()
    assert L.mrg_job_map_add(None) == native.EINVAL
    assert b"null context" in L.mrg_last_error()
    b, p = native.run_stream_stats()        # no job yet on this thread, or whatever the last one left
    assert b >= 0 and p >= 0
    assert L.mrg_run_get_stream_stats(None, None) == 0
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    f = tmp_path / "a.txt"
    f.write_bytes(b"a b c\n")
    with pytest.raises(native.MrgError) as ei:
        native.run_job([str(f)], 2, native.APP_WC, str(tmp_path), native.FLAG_STREAM)
    assert ei.value.code == native.EHIP


def test_constants_agree():
    from mapreduce_rust_amd import native
    hdr = open(os.path.join(ROOT, "include", "mrgpu.h")).read()
    rs = open(os.path.join(ROOT, "mrgpu-sys", "src", "lib.rs")).read()
    assert re.search(r"^#define MRG_FLAG_STREAM 0x4u\b", hdr, re.M)
    assert native.FLAG_STREAM == 0x4
    assert "pub const MRG_FLAG_STREAM: u32 = 0x4;" in rs
    assert "#define MRG_ABI_VERSION 6" in hdr and native.ABI_VERSION == 6
    # mrg_stats.reserved became map_batches: the last field, same size and offset
    assert native.Stats._fields_[-1] == ("map_batches", C.c_uint32)
    assert C.sizeof(native.Stats) == 160 and native.Stats.map_batches.offset == 156
    assert re.search(r"uint32_t map_batches;", hdr.split("} mrg_stats;")[0])
    assert "pub map_batches: u32," in rs.split("pub struct mrg_stats")[1].split("}")[0]
    assert "reserved" not in [f for f, _ in native.Stats._fields_]
    for sym in ("mrg_job_map_add", "mrg_run_get_stream_stats"):
        assert sym in native.exported_symbols() and "pub fn %s(" % sym in rs
        assert hasattr(native.load(), sym), sym
    assert hasattr(native.load(), "mrg_test_stream_plan") and "mrg_test_stream_plan" not in hdr
    assert callable(native.Context.map_add)
