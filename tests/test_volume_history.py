"""The edit history (vrt_volume_history, vrt.h) without a GPU: the info struct has the C layout, and the numpy model that
tests/test_volume_history_gpu.py holds the device to (tests/history_ref.py) agrees with itself — undoing every entry of a session gives
its first state in bits, a redo gives the last one back, hand-made 9^3 changes touch the tiles they must, and the limits rule drops
what the contract says it drops."""
import ctypes as C
import os
import subprocess

import numpy as np

import history_ref as H
import session_model as M
from volumetricraytracer_amd import _abi
from test_volume_session import SEEDS, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_info_struct_is_64_bytes_in_c_and_in_ctypes(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vrt.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(vrt_history_info), offsetof(vrt_history_info, max_bytes),'
                    " offsetof(vrt_history_info, bytes), offsetof(vrt_history_info, top_tiles), offsetof(vrt_history_info, reserved_),"
                    " VRT_HISTORY_TILE, VRT_HISTORY_TILE_BYTES);return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    info = _abi.vrt_history_info
    assert got == [C.sizeof(info), info.max_bytes.offset, info.bytes.offset, info.top_tiles.offset, info.reserved_.offset,
                   _abi.HISTORY_TILE, _abi.HISTORY_TILE_BYTES]
    assert got[0] == 64 and (H.TILE, H.TILE_BYTES) == (got[5], got[6])
    assert H.TILE_BYTES >= 64 * 4 + 64 + 4 and H.TILE_BYTES % 16 == 0  # bits, ids and key, padded


def runs_of(steps, slot):
    """The states of a slot between two uploads or frees, as lists of (stored, material): what one history can span."""
    runs, run = [], []
    for s in steps:
        m = s["after"][slot]
        if s["slot"] == slot and s["kind"] in ("upload", "free"):
            runs.append(run)
            run = []
        if m.used and s["slot"] == slot and s["kind"] in ("upload",) + M.EDITS:
            run.append((m.stored, m.material))
    return [r for r in runs + [run] if len(r) > 1]


def test_undoing_every_entry_of_a_session_gives_its_first_state():
    n_entries = 0
    for seed in SEEDS:
        for slot in M.SLOTS:
            for run in runs_of(M.program(seed), slot):
                h = H.History(1000, 1 << 40)
                for before, after in zip(run, run[1:]):
                    tiles = h.record(before, after)
                    differ = (H.bits_of(before[0]) != H.bits_of(after[0])) | (before[1] != after[1])
                    assert (tiles > 0) == bool(differ.any())
                    assert tiles * 64 >= int(differ.sum())
                assert h.info()["bytes"] == sum(len(e) for e in h.undo) * H.TILE_BYTES and not h.redo
                k = len(h.undo)
                n_entries += k
                d, m, got = h.undo_steps(run[-1], k)
                assert same_bits(d, run[0][0]) and np.array_equal(m, run[0][1]), (seed, slot)
                assert len(h.redo) == k and not h.undo and got["written"] >= 1
                d, m, again = h.redo_steps((d, m), k)
                assert same_bits(d, run[-1][0]) and np.array_equal(m, run[-1][1]), (seed, slot)
                assert again["written"] == got["written"] and (again["lo"], again["hi"]) == (got["lo"], got["hi"])
    assert n_entries > 30


def field9():
    rng = np.random.default_rng(9)
    return rng.standard_normal((9, 9, 9)).astype(np.float32), rng.integers(0, 4, (9, 9, 9)).astype(np.uint8)


def test_tiles_of_hand_made_changes_on_9_cubed():
    d0, m0 = field9()
    d1, m1 = d0.copy(), m0.copy()
    d1[8, 8, 8] = np.float32(7.0)       # only in the last tile of every axis, which is one sample thick
    m1[0, 0, 3], m1[0, 0, 4] = 9, 9     # ids only, straddling two tiles along y
    tiles = H.changed_tiles((d0, m0), (d1, m1))
    assert tiles.tolist() == [[0, 0, 0], [0, 0, 1], [2, 2, 2]]
    assert H.keys_of(9, tiles).tolist() == [0, 1, 26] and H.tiles_per_axis(9) == 3
    h = H.History(4, 1 << 20)
    assert h.record((d0, m0), (d1, m1)) == 3 and h.info()["top_tiles"] == 3 and h.info()["bytes"] == 3 * H.TILE_BYTES
    d, m, got = h.undo_steps((d1, m1))
    assert same_bits(d, d0) and np.array_equal(m, m0)
    assert got == {"written": 3, "lo": (0, 3, 0), "hi": (8, 8, 8)}
    # bits, not values: -0.0 against +0.0 is a change, one NaN payload against another too; a value against itself is none
    d2 = d0.copy()
    d0z = d0.copy()
    d0z[1, 1, 1], d2[1, 1, 1] = np.float32(0.0), np.float32(-0.0)
    d0z.view(np.uint32)[5, 5, 5], d2.view(np.uint32)[5, 5, 5] = 0x7FC00001, 0x7FC00002
    assert H.changed_tiles((d0z, m0), (d2, m0)).tolist() == [[0, 0, 0], [1, 1, 1]]
    assert h.record((d0, m0), (d0.copy(), m0.copy())) == 0 and len(h.redo) == 1  # no bit changed: nothing recorded, redo kept


def test_the_limits_rule_on_a_scripted_sequence():
    N = 17
    base = np.zeros((N, N, N), np.float32), np.zeros((N, N, N), np.uint8)

    def dab(state, x, n_tiles=1):
        d = state[0].copy()
        for t in range(n_tiles):
            d[x, 0, 4 * t] += np.float32(1.0)
        return d, state[1]

    h = H.History(2, 10 * H.TILE_BYTES)
    s = [base]
    for x in (0, 4, 8):
        s.append(dab(s[-1], x))
        h.record(s[-2], s[-1])
    assert (len(h.undo), h.dropped, h.bytes) == (2, 1, 2 * H.TILE_BYTES)  # the third entry dropped the first
    d, m, _ = h.undo_steps(s[-1], 2)
    assert same_bits(d, s[1][0])  # back to after the first dab, which can no longer be undone
    d, m, _ = h.redo_steps((d, m), 1)
    assert (len(h.undo), len(h.redo)) == (1, 1)
    s2 = dab((d, m), 12, 4)
    h.record((d, m), s2)  # a new edit empties the redo stack, uncounted
    assert (len(h.undo), len(h.redo), h.dropped, h.bytes) == (2, 0, 1, 5 * H.TILE_BYTES)
    h.set_limits(8, 10 * H.TILE_BYTES)
    s3 = dab(s2, 16, 4)
    s4 = dab(s3, 2, 4)
    h.record(s2, s3)
    assert (len(h.undo), h.dropped, h.bytes) == (3, 1, 9 * H.TILE_BYTES)
    h.record(s3, s4)  # 13 tiles: over the bytes; the oldest goes until they hold
    assert (len(h.undo), h.dropped, h.bytes) == (2, 3, 8 * H.TILE_BYTES)
    big = (s4[0] + np.float32(1.0), s4[1])  # every tile: more than the history may hold on its own
    assert h.record(s4, big) == 125
    assert (len(h.undo), len(h.redo), h.dropped, h.bytes, h.info()["top_tiles"]) == (0, 0, 6, 0, 0)
    assert (h.max_entries, h.max_bytes) == (8, 10 * H.TILE_BYTES)
    # lowering the limits of a history that is on: undo entries first, then the redo entries furthest ahead
    h = H.History(8, 100 * H.TILE_BYTES)
    s = [base]
    for x in (0, 4, 8, 12):
        s.append(dab(s[-1], x))
        h.record(s[-2], s[-1])
    state = h.undo_steps(s[-1], 3)[:2]
    h.set_limits(8, 2 * H.TILE_BYTES)
    assert (len(h.undo), len(h.redo), h.dropped) == (0, 2, 2)
    d, m, _ = h.redo_steps(state, 2)
    assert same_bits(d, s[3][0])  # the two nearest redo entries were kept
    h.clear()
    assert h.info()["dropped"] == 2 and h.bytes == 0
