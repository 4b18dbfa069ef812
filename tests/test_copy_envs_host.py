"""pom_batch_copy_envs without a GPU: the header declares it, and the per-env column movement its kernels use (pom_packed.h
pom_col_copy_item / pom_rec_to_col_item / pom_col_to_rec_item) compiled for the host and checked byte for byte against the tile
layout written out in numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.host_build import ROOT, shared_lib

TILE_DWORDS, REC_DWORDS, BOARD_BYTES = 1280, 80, 124

HARNESS = r"""
#include "pom_packed.h"
extern "C" {
void h_col_copy(uint32_t* dst_tile, int dst_lane, const uint32_t* src_tile, int src_lane) { pom_col_copy(dst_tile, dst_lane, src_tile, src_lane); }
void h_rec_to_col(uint32_t* dst_tile, int dst_lane, const uint32_t* rec) { pom_rec_to_col(dst_tile, dst_lane, rec); }
void h_col_to_rec(uint32_t* rec, const uint32_t* src_tile, int src_lane, int as_snapshot) { pom_col_to_rec(rec, src_tile, src_lane, as_snapshot != 0); }
int h_items(void) { return POM_COL_ITEMS; }
}
"""


@pytest.fixture(scope="module")
def helpers(tmp_path_factory):
    src = tmp_path_factory.mktemp("copy_helpers") / "copy_helpers.cpp"
    src.write_text(HARNESS)
    h = C.CDLL(shared_lib(str(src)))
    h.h_col_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    h.h_rec_to_col.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    h.h_col_to_rec.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    return h


def _column(tile: np.ndarray, lane: int):
    """env `lane`'s column of a tile as (124 board bytes, dwords 31..79): board cell c at byte c * 16 + lane, dword d at d * 16 + lane"""
    return tile.view(np.uint8)[:BOARD_BYTES * 16].reshape(BOARD_BYTES, 16)[:, lane].copy(), tile.reshape(REC_DWORDS, 16)[31:, lane].copy()


def _record(rec: np.ndarray):
    return rec.view(np.uint8)[:BOARD_BYTES].copy(), rec[31:].copy()


def _others_unchanged(after: np.ndarray, before: np.ndarray, lane: int):
    for other in range(16):
        if other != lane:
            a, b = _column(after, other), _column(before, other)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), other
    # the two bytes past the board rows' 124 cells do not exist: the board is 31 rows of 64 B = 124 cells x 16 envs
    assert after.size == before.size == TILE_DWORDS


def test_header_declares_copy_entry_points():
    text = open(os.path.join(ROOT, "include", "pom_batch.h")).read()
    assert re.search(r"int pom_batch_copy_envs\(PomBatch\* h, const int64_t\* src_host, int64_t first, int64_t count, int32_t flags\);", text)
    assert re.search(r"int pom_batch_copy_envs_device\(PomBatch\* h, const int64_t\* src_dev, int64_t first, int64_t count, int32_t flags\);", text)
    assert re.search(r"POM_COPY_FROM_SNAPSHOT\s*=\s*1", text) and re.search(r"POM_COPY_SET_SNAPSHOT\s*=\s*2", text)
    hpp = open(os.path.join(ROOT, "include", "pom_bboard.hpp")).read()
    assert "void CopyGames(" in hpp and "void CopyGamesDevice(" in hpp


def test_item_count(helpers):
    assert helpers.h_items() == BOARD_BYTES + (REC_DWORDS - 31)


def test_tile_to_tile_column(helpers):
    rng = np.random.default_rng(3)
    for _ in range(64):
        src = rng.integers(0, 2**32, TILE_DWORDS, dtype=np.uint32)
        dst = rng.integers(0, 2**32, TILE_DWORDS, dtype=np.uint32)
        sl, dl = (int(v) for v in rng.integers(0, 16, 2))
        before = dst.copy()
        helpers.h_col_copy(dst.ctypes.data, dl, src.ctypes.data, sl)
        got, want = _column(dst, dl), _column(src, sl)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        _others_unchanged(dst, before, dl)
        assert np.array_equal(src.reshape(80, 16)[:, sl], src.reshape(80, 16)[:, sl])  # (source untouched by construction)


def test_same_tile_column_copy(helpers):
    """a source column in the destination's own tile (what K1 sees when a source lies next to its destination)"""
    rng = np.random.default_rng(4)
    t = rng.integers(0, 2**32, TILE_DWORDS, dtype=np.uint32)
    before = t.copy()
    helpers.h_col_copy(t.ctypes.data, 9, t.ctypes.data, 2)
    got, want = _column(t, 9), _column(before, 2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    _others_unchanged(t, before, 9)


def test_record_to_column_and_back(helpers):
    rng = np.random.default_rng(5)
    for _ in range(64):
        rec = rng.integers(0, 2**32, REC_DWORDS, dtype=np.uint32)
        dst = rng.integers(0, 2**32, TILE_DWORDS, dtype=np.uint32)
        lane = int(rng.integers(0, 16))
        before = dst.copy()
        helpers.h_rec_to_col(dst.ctypes.data, lane, rec.ctypes.data)
        got, want = _column(dst, lane), _record(rec)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        _others_unchanged(dst, before, lane)
        back = np.zeros(REC_DWORDS, dtype=np.uint32)
        helpers.h_col_to_rec(back.ctypes.data, dst.ctypes.data, lane, 0)
        assert np.array_equal(back, rec)
        # as a snapshot: status and ubflags (top bytes of agent words 35, 37, 39 = bytes 1..3 of meta2) come out clear, nothing else moves
        snap = np.zeros(REC_DWORDS, dtype=np.uint32)
        helpers.h_col_to_rec(snap.ctypes.data, dst.ctypes.data, lane, 1)
        want_snap = rec.copy()
        want_snap[[35, 37, 39]] &= 0x00FFFFFF
        assert np.array_equal(snap, want_snap)


def test_partial_last_tile(helpers):
    """n = 100 envs in 7 tiles: copies into the last tile's four real columns leave the twelve blank columns past n blank"""
    n, n_pad = 100, 112
    rng = np.random.default_rng(6)
    buf = rng.integers(0, 2**32, n_pad * REC_DWORDS, dtype=np.uint32).reshape(n_pad // 16, TILE_DWORDS)
    buf[-1] = 0
    last = buf[-1]
    for e in range(96, n):  # the real columns of the last tile hold something
        helpers.h_rec_to_col(last.ctypes.data, e % 16, rng.integers(0, 2**32, REC_DWORDS, dtype=np.uint32).ctypes.data)
    before = buf.copy()
    src = [3, 99, 50, 97]  # env 96 + i <- env src[i]: from other tiles and from the last tile itself
    recs = {}
    for s in set(src):
        t = np.ascontiguousarray(before[s // 16])
        r = np.zeros(REC_DWORDS, dtype=np.uint32)
        helpers.h_col_to_rec(r.ctypes.data, t.ctypes.data, s % 16, 0)
        recs[s] = r
    for i, s in enumerate(src):  # through records: every source read before any destination is written
        helpers.h_rec_to_col(last.ctypes.data, (96 + i) % 16, recs[s].ctypes.data)
    for i, s in enumerate(src):
        got, want = _column(last, (96 + i) % 16), _column(np.ascontiguousarray(before[s // 16]), s % 16)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (i, s)
    for lane in range(n - 96, 16):
        b, d = _column(last, lane)
        assert not b.any() and not d.any(), lane
    assert np.array_equal(buf[:-1], before[:-1])
