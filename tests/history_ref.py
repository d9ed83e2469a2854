"""A numpy model of a slot's edit history (vrt_volume_history, vrt.h), on top of the stored arrays of volume_ref / session_model states:
two stacks of entries (tile keys, the tiles' stored bits and ids as they were), the changed tiles of a before/after pair, the limits
rule, and what an undo or redo of k entries reports.  Arrays are indexed [x, z, y] like the grid; everything compares bits.  Written
from the contract in vrt.h, not from the kernels: tiles are found on zero-padded arrays, all at once."""
from __future__ import annotations

import numpy as np

TILE = 4
TILE_BYTES = 336  # 64 x 4 B of bits + 64 B of ids + 4 B of key, padded to 16: VRT_HISTORY_TILE_BYTES


def bits_of(stored) -> np.ndarray:
    return np.ascontiguousarray(stored, np.float32).view(np.uint32)


def tiles_per_axis(N: int) -> int:
    return (N + TILE - 1) // TILE


def _tiled(a: np.ndarray) -> np.ndarray:
    """[N, N, N] -> [T, T, T, 4, 4, 4] (a copy), zero beyond the grid."""
    N = a.shape[0]
    T = tiles_per_axis(N)
    p = np.zeros((T * TILE,) * 3, a.dtype)
    p[:N, :N, :N] = a
    return np.ascontiguousarray(p.reshape(T, TILE, T, TILE, T, TILE).transpose(0, 2, 4, 1, 3, 5))


def _untiled(t: np.ndarray, N: int) -> np.ndarray:
    T = t.shape[0]
    return np.ascontiguousarray(t.transpose(0, 3, 1, 4, 2, 5).reshape((T * TILE,) * 3)[:N, :N, :N])


def changed_tiles(before, after) -> np.ndarray:
    """before, after: (stored, material).  The tile coordinates [k, 3] = (tx, tz, ty), in key order, of the aligned 4^3 tiles with at
    least one sample whose density bits or id differ."""
    differ = (bits_of(before[0]) != bits_of(after[0])) | (np.asarray(before[1]) != np.asarray(after[1]))
    return np.argwhere(_tiled(differ).any(axis=(3, 4, 5)))


def keys_of(N: int, tiles: np.ndarray) -> np.ndarray:
    T = tiles_per_axis(N)
    return (tiles[:, 0] * T + tiles[:, 1]) * T + tiles[:, 2]


class Entry:
    def __init__(self, tiles, bits, ids):
        self.tiles, self.bits, self.ids = tiles, bits, ids  # [k, 3], [k, 4, 4, 4] uint32, [k, 4, 4, 4] uint8

    def __len__(self):
        return len(self.tiles)


def swap(entry: Entry, stored, material):
    """Exchanges the entry's tiles with the volume's.  Returns (stored, material, samples changed, changed mask [N, N, N]); the entry
    now holds what the volume held."""
    N = stored.shape[0]
    d, m = _tiled(bits_of(stored)), _tiled(np.asarray(material, np.uint8))
    at = tuple(entry.tiles.T)
    held_d, held_m = d[at].copy(), m[at].copy()
    differ = np.zeros(d.shape, bool)
    differ[at] = (held_d != entry.bits) | (held_m != entry.ids)
    d[at], m[at] = entry.bits, entry.ids
    entry.bits, entry.ids = held_d, held_m
    mask = _untiled(differ, N)
    assert int(mask.sum()) == int(differ.sum())  # the padding never differs: it is zero on both sides
    return _untiled(d, N).view(np.float32), _untiled(m, N), int(mask.sum()), mask


def box_of(mask: np.ndarray):
    """(lo, hi) in xyz, inclusive, of the set samples of a mask [x, z, y]; lo > hi when none."""
    N = mask.shape[0]
    if not mask.any():
        return (N, N, N), (-1, -1, -1)
    x, z, y = np.nonzero(mask)
    return (int(x.min()), int(y.min()), int(z.min())), (int(x.max()), int(y.max()), int(z.max()))


class History:
    """The stacks of one slot.  `undo` holds the oldest entry first; `redo` holds the entry a redo takes next last."""

    def __init__(self, max_entries: int, max_bytes: int):
        assert max_entries > 0 and max_bytes > 0
        self.max_entries, self.max_bytes = max_entries, max_bytes
        self.undo, self.redo, self.dropped = [], [], 0

    @property
    def bytes(self) -> int:
        return sum(len(e) for e in self.undo + self.redo) * TILE_BYTES

    def info(self) -> dict:
        return {"enabled": 1, "max_entries": self.max_entries, "max_bytes": self.max_bytes, "undo_entries": len(self.undo),
                "redo_entries": len(self.redo), "bytes": self.bytes, "dropped": self.dropped,
                "top_tiles": len(self.undo[-1]) if self.undo else 0}

    def _trim(self):
        while len(self.undo) > self.max_entries or self.bytes > self.max_bytes:
            if self.undo:
                self.undo.pop(0)
            elif self.redo:
                self.redo.pop(0)  # the one furthest ahead
            else:
                break
            self.dropped += 1

    def set_limits(self, max_entries: int, max_bytes: int):
        self.max_entries, self.max_bytes = max_entries, max_bytes
        self._trim()

    def clear(self):
        """An upload onto the slot: the entries go, uncounted; the limits stay."""
        self.undo, self.redo = [], []

    def record(self, before, after) -> int:
        """A recording call took (stored, material) from `before` to `after`.  Returns the changed tiles; 0 records nothing."""
        tiles = changed_tiles(before, after)
        if len(tiles) == 0:
            return 0
        self.redo = []
        if len(tiles) * TILE_BYTES > self.max_bytes:  # larger than the history may be: everything goes, the new entry too
            self.dropped += len(self.undo) + 1
            self.undo = []
            return len(tiles)
        at = tuple(tiles.T)
        self.undo.append(Entry(tiles, _tiled(bits_of(before[0]))[at], _tiled(np.asarray(before[1], np.uint8))[at]))
        self._trim()
        return len(tiles)

    def _step(self, state, k: int, src: list, dst: list):
        assert 1 <= k <= len(src)
        stored, material = state
        written, touched = 0, np.zeros(stored.shape, bool)
        for _ in range(k):
            entry = src.pop()
            stored, material, n, mask = swap(entry, stored, material)
            written += n
            touched |= mask
            dst.append(entry)
        lo, hi = box_of(touched)
        return stored, material, {"written": written, "lo": lo, "hi": hi}

    def undo_steps(self, state, k: int = 1):
        """(stored, material, {"written", "lo", "hi"}) after taking the k newest undo entries, newest first."""
        return self._step(state, k, self.undo, self.redo)

    def redo_steps(self, state, k: int = 1):
        return self._step(state, k, self.redo, self.undo)
