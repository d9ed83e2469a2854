"""One model of a context's two volume slots, and seeded programs of calls over them: what tests/test_volume_session.py (host passes)
and tests/test_volume_session_gpu.py (device) share.  The model composes the numpy references of the single calls (tests/*_ref.py and
volume_ref.device_bytes) and adds no arithmetic of its own; what it adds is the state a context carries from one call to the next: each
slot's grid, format and metric, whether it is used, and the rule of vrt_volume_upload for a slot that was used before.

program(seed) draws the calls and runs the model along: every step carries the record the API must report and a snapshot of both slots
after it.  coverage(program) counts, from the model alone, what the program is for."""
from __future__ import annotations

import copy
import functools
import math

import numpy as np

import brush_ref as B
import components_ref as CR
import fill_ref as F
import mesh_ref as MR
import redistance_ref as RR
import smooth_ref as S
import stamp_ref as ST
import volume_ref as R
import volumetricraytracer_amd as v
import warp_ref as W
from volumetricraytracer_amd import _abi

SLOTS = (0, 1)
EXTENTS = (100.0, 60.0)
SCALES = (1.0, 0.37)
STEPS_ON = (0.5, 1.5, math.inf)  # step_max in cells (inf as it is): the tables on
STEPS_OFF = (0.0, -1.0)          # step_max itself: the tables off
BANDS = (1, 3, 8)
FROMS = (RR.BOTH, RR.OUTSIDE, RR.INSIDE)
EDITS = ("update_region", "brushes", "stamp", "smooth", "warp", "fill", "components", "redistance")
READS = ("extract_mesh", "download_region", "download_volume")
KINDS = ("upload", "free", "set_metric") + EDITS + READS
REFUSED = "refused"  # what a components call wants that must end in VRT_ERR_INVALID after the device was read
VOXEL = np.dtype([("material", "u1"), ("pad", "u1", 3), ("density", "<f4")])


def _frozen(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


class SlotModel:
    """One slot as the context holds it.  A call is a method on a copy (the arrays are read-only and shared, never written in place):
    it applies the call's reference and returns the record the API must report."""

    def __init__(self):
        self.used = False
        self.res = self.N = self.extent = self.fmt = self.stored = self.material = None
        self.scale, self.step = 1.0, 0.0
        self._bytes = None

    def copy(self) -> "SlotModel":
        return copy.copy(self)

    def _set(self, stored=None, material=None):
        if stored is not None:
            self.stored = _frozen(stored, np.float32)
        if material is not None:
            self.material = _frozen(material, np.uint8)
        self._bytes = None

    @property
    def unit(self):
        return B.units(self.N, self.extent, self.scale)[1]

    @property
    def tables(self) -> bool:
        return self.step > 0

    def expected_buffers(self) -> dict:
        """What vrt_debug_volume_bytes must return for the slot; 'active_box' is None without the tables (the slot keeps the box it had)."""
        if self._bytes is None:
            self._bytes = R.device_bytes(self.stored, self.material, self.fmt, self.scale, self.step)
        return self._bytes

    def decoded(self) -> np.ndarray:
        """What vrt_volume_download* hands out."""
        return B.decode(self.stored, self.fmt)

    # -- calls ---------------------------------------------------------------------------------------------------------------------
    def upload(self, res, extent, fmt, path, density=None, material=None, records=None, texels=None):
        """vrt_volume_upload / _upload_voxels / _upload_texels.  A slot that was used keeps its metric; a free one starts from (1, 0)."""
        N = (1 << res) + 1
        if path == "texels":
            assert fmt == R.TEXEL16
            stored, ids = R.decode_texels(texels)
        elif path == "voxels":
            d, ids = R.split_records(records)
            stored, ids = R.dense_field(d.reshape(N, N, N), fmt), ids.reshape(N, N, N)
        else:
            stored = R.dense_field(density, fmt)
            ids = np.zeros((N, N, N), np.uint8) if path == "float_nomat" else material
        if not self.used:
            self.scale, self.step = 1.0, 0.0
        self.used, self.res, self.N, self.extent, self.fmt = True, res, N, float(extent), fmt
        self._set(stored, ids)

    def free(self):
        self.__init__()

    def set_metric(self, scale, step):
        self.scale, self.step = float(scale), float(step)
        self._bytes = None

    def update_region(self, origin, values, material=None):
        """vrt_volume_update_region / _update_voxels: values [sx, sz, sy] at origin xyz; material None keeps the ids."""
        x0, y0, z0 = origin
        sx, sz, sy = values.shape
        box = (slice(x0, x0 + sx), slice(z0, z0 + sz), slice(y0, y0 + sy))
        d, m = np.array(self.stored), np.array(self.material)
        d[box] = R.dense_field(values, self.fmt)
        if material is not None:
            m[box] = material
        self._set(d, m)

    def brushes(self, records) -> dict:
        d, m = np.array(self.stored), np.array(self.material)
        got = B.apply(d, m, self.fmt, records, self.extent, self.scale)
        self._set(d, m)
        return got

    def stamp(self, src: "SlotModel", rec) -> dict:
        d, m = np.array(self.stored), np.array(self.material)
        got = ST.apply(d, m, self.fmt, self.extent, self.scale, src.stored, src.material, src.fmt, src.extent, src.scale, rec)
        self._set(d, m)
        return got

    def smooth(self, rec) -> dict:
        d, m, got = S.smooth(self.stored, self.material, self.fmt, rec)
        self._set(d, m)
        return got

    def warp(self, rec) -> dict:
        d, m, got, density_writes = W.warp(self.stored, self.material, self.fmt, rec, self.extent, self.scale)
        self._set(d, m)
        return dict(got, density_writes=density_writes)

    def fill(self, wall, material) -> dict:
        d, m, got = F.fill(self.stored, self.material, self.fmt, wall, material)
        self._set(d, m)
        return got

    def components(self, list_capacity=0, **kw):
        """The result record, or REFUSED (and nothing changed) for a seed without a solid sample around it."""
        try:
            d, m, got = CR.components(self.stored, self.material, self.fmt, list_capacity=list_capacity, **kw)
        except CR.NoSolidSampleAtSeed:
            return REFUSED
        self._set(d, m)
        return got

    def redistance(self, band, from_, lo=None, hi=None) -> dict:
        d, got = RR.redistance(self.stored, self.fmt, band, from_, self.unit, lo, hi)
        self._set(d)
        return got

    # -- read-only calls -----------------------------------------------------------------------------------------------------------
    def extract_mesh(self, iso=0.0, lo=None, hi=None):
        return MR.extract(self.stored, self.material, self.fmt, iso, self.extent, lo, hi)

    def download_region(self, lo, hi):
        box = (slice(lo[0], hi[0] + 1), slice(lo[2], hi[2] + 1), slice(lo[1], hi[1] + 1))
        return self.decoded()[box], self.material[box]

    def download_volume(self):
        return self.decoded(), self.material


def wrote(kind: str, want) -> bool:
    """Whether an editing call wrote at least one sample, from the record it must report."""
    if kind == "update_region":
        return True
    if want == REFUSED:
        return False
    return (want["filled"] if kind == "fill" else want["written"]) > 0


def same_record(kind: str, got, want) -> bool:
    """The reported record against the model's: equal — but for an empty box, which only has to be empty (lo > hi on every axis), a
    fill's round count, which is the device's own, and the warp's count of density writes, which the API does not report."""
    if want == REFUSED or got == REFUSED:
        return got == want
    want = {k: w for k, w in want.items() if k not in ("sweeps", "density_writes")}
    got = {k: g for k, g in got.items() if k != "sweeps"}
    count = "filled" if kind == "fill" else "written"
    if kind in ("brushes", "stamp", "smooth", "warp", "fill") and want[count] == 0:
        return got[count] == 0 and all(l > h for l, h in zip(got["lo"], got["hi"]))
    return got == want


# ---- fields ------------------------------------------------------------------------------------------------------------------------------

def analytic_field(rng, N: int, extent: float, shape: str):
    """(density, material): a sphere or a torus about the grid's centre (off the lattice) as a distance in object units, ids that
    differ from sample to sample inside it — and, where the grid has room, the NaN, +0 and -0 samples of extreme_cases.random_field at
    their places, and a +inf and a -inf sample."""
    cell = 2.0 * extent / (N - 1)
    i = np.arange(N, dtype=np.float64)
    x, z, y = i[:, None, None], i[None, :, None], i[None, None, :]
    c = (N - 1) / 2.0 + rng.uniform(-0.4, 0.4, 3)
    dx, dy, dz = x - c[0], y - c[1], z - c[2]
    if shape == "sphere":
        d = np.sqrt(dx * dx + dy * dy + dz * dz) - 0.33 * (N - 1)
    else:
        q = np.sqrt(dx * dx + dy * dy) - 0.28 * (N - 1)
        d = np.sqrt(q * q + dz * dz) - 0.15 * (N - 1)
    d = (d * cell).astype(np.float32)
    ids = np.where(d <= 0, 1 + (x * 3 + y * 5 + z * 7) % 5, 0).astype(np.uint8)
    if N >= 5:
        d[1, 1, 1], d[0, 2, 1], d[2, 0, 1] = np.float32(np.nan), np.float32(0.0), np.float32(-0.0)
        d[N - 2, 1, 2], d[1, N - 2, 2] = np.float32(np.inf), np.float32(-np.inf)
    return d, ids


def quat(axis, degrees: float):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = math.radians(degrees) / 2.0
    return tuple(a * math.sin(h)) + (math.cos(h),)


# ---- the program ---------------------------------------------------------------------------------------------------------------------------

class _Generator:
    """Draws the steps of a program and runs the model along."""

    def __init__(self, seed: int, formats):
        self.rng = np.random.default_rng(1000 + seed)
        self.seed = seed
        self.formats = tuple(formats)
        self.m = [SlotModel(), SlotModel()]
        self.steps = []
        self.last_box = {}
        self.uploads = {}
        self.turns = {}  # per kind of choice: cycles shapes, ops, bands and modes so that a few calls cover them all

    def next_turn(self, what: str) -> int:
        self.turns[what] = self.turns.get(what, self.seed - 1) + 1
        return self.turns[what]

    def step(self, kind, slot, want=None, new=None, **args):
        if new is not None:
            self.m[slot] = new
        if kind in EDITS and want not in (None, REFUSED) and wrote(kind, want) and "lo" in want:
            self.last_box[slot] = (want["lo"], want["hi"])
        self.steps.append({"kind": kind, "slot": slot, "args": args, "want": want, "after": tuple(self.m), "n": len(self.steps)})

    def other_format(self, fmt):
        return next((f for f in self.formats if f != fmt), fmt)

    # -- state changes -----------------------------------------------------------------------------------------------------------------
    def upload(self, slot, res, fmt, path=None):
        rng = self.rng
        N = (1 << res) + 1
        extent = EXTENTS[slot]
        d, ids = analytic_field(rng, N, extent, ("sphere", "torus")[self.next_turn("upload") % 2])
        if path is None:  # every path a format has, in turn
            paths = ("texels", "float", "voxels", "float_nomat")[fmt != R.TEXEL16:]
            self.uploads[fmt] = self.uploads.get(fmt, -1) + 1
            path = paths[(self.uploads[fmt] + (self.seed if fmt != R.TEXEL16 else 0)) % len(paths)]
        args = dict(res=res, extent=extent, fmt=fmt, path=path)
        if path == "texels":
            args["texels"] = _frozen(B.texels_of(R.texel16_field(d), ids), np.uint8)
        elif path == "voxels":
            rec = np.zeros(N ** 3, VOXEL)
            rec["density"], rec["material"] = d.reshape(-1), ids.reshape(-1)
            args["records"] = rec
        else:
            args["density"], args["material"] = _frozen(d, np.float32), _frozen(ids, np.uint8)
        new = self.m[slot].copy()
        new.upload(**args)
        self.last_box.pop(slot, None)
        self.step("upload", slot, None, new, **args)

    def free(self, slot):
        new = self.m[slot].copy()
        new.free()
        self.last_box.pop(slot, None)
        self.step("free", slot, None, new)

    def set_metric(self, slot, tables: bool):
        m = self.m[slot]
        cell = 2.0 * m.extent / (m.N - 1)
        t = self.next_turn("set_metric")
        scale = SCALES[t % 2]
        if tables:
            f = STEPS_ON[t % 3]
            step = f if math.isinf(f) else float(np.float32(f * cell))
        else:
            step = STEPS_OFF[t % 2]
        if (scale, step) == (m.scale, m.step):
            scale = SCALES[(t + 1) % 2]
        new = m.copy()
        new.set_metric(scale, step)
        self.step("set_metric", slot, None, new, scale=scale, step=step)

    # -- edits -------------------------------------------------------------------------------------------------------------------------
    def update_region(self, slot, records: bool):
        m, rng = self.m[slot], self.rng
        N = m.N
        size = [int(rng.integers(1, max(2, N // 2))) for _ in range(3)]
        origin = [int(rng.integers(0, N - s + 1)) for s in size]
        sx, sy, sz = size
        cell = 2.0 * m.extent / (N - 1)
        values = (rng.standard_normal((sx, sz, sy)) * 2.0 * cell).astype(np.float32)
        flat = values.reshape(-1)
        for k, special in enumerate((np.nan, 0.0, -0.0)):
            if flat.size > k + 1:
                flat[(k * 7 + 1) % flat.size] = np.float32(special)
        ids = rng.integers(0, 6, values.shape).astype(np.uint8) if records or self.next_turn("update_region") % 2 else None
        self._update(slot, origin, values, ids, records)

    def _update(self, slot, origin, values, ids, records):
        new = self.m[slot].copy()
        new.update_region(tuple(origin), values, ids)
        self.step("update_region", slot, None, new, origin=tuple(origin), values=_frozen(values, np.float32),
                  material=None if ids is None else _frozen(ids, np.uint8), records=records)

    def zero_box(self, slot):
        """A box of +0 densities (solid) with ids that differ from sample to sample about the centre: what an ids-only warp moves."""
        N = self.m[slot].N
        h = min(5, (N - 1) // 2 - 1)
        c = (N - 1) // 2
        n = 2 * h + 1
        values = np.zeros((n, n, n), np.float32)
        i = np.arange(n)
        ids = (1 + (i[:, None, None] * 3 + i[None, :, None] * 5 + i[None, None, :] * 7) % 11).astype(np.uint8)
        self._update(slot, (c - h,) * 3, values, ids, True)

    def brushes(self, slot, outside: bool = False):
        m, rng = self.m[slot], self.rng
        N = m.N
        c = (N - 1) / 2.0
        recs = []
        for _ in range(int(rng.integers(1, 3)) if outside else int(rng.integers(1, 4))):
            t = self.next_turn("brushes")
            shape, op = t % 3, (t // 3 + t) % 3
            way = rng.standard_normal(3)
            way /= np.linalg.norm(way)
            at = c + way * 0.33 * (N - 1)
            if t % 4 == 0:  # across a face
                at[t % 3] = N - 1 + 0.3
            r = float(rng.uniform(0.1, 0.2) * (N - 1) + 0.6)
            blend, material = (0.0, 1.5)[t % 2], (-1, 3, 7)[t % 3] if op != B.PAINT else 9
            if shape == B.SPHERE:
                recs.append(v.sphere_brush(op, tuple(at), r, blend, 2.0, material))
            elif shape == B.BOX:
                recs.append(v.box_brush(op, tuple(at), (r, 0.7 * r, 1.2 * r), 0.3 * r, blend, 2.0, material))
            else:
                recs.append(v.capsule_brush(op, tuple(at), tuple(at - way * 0.3 * (N - 1)), 0.6 * r, blend, 2.0, material))
        if outside:
            recs.append(v.sphere_brush(B.ADD, (-4.0 * N, c, c), 1.0, 0.0, 1.0, 2))
        self._brushes(slot, recs)

    def _brushes(self, slot, recs):
        new = self.m[slot].copy()
        want = new.brushes(recs)
        self.step("brushes", slot, want, new, records=recs)

    def cavity(self, slot):
        """A hard SUBTRACT ball wholly inside the solid, about its deepest sample: a cavity for the fill."""
        m = self.m[slot]
        d = np.array(m.decoded(), np.float64)
        core = CR.solid(m.decoded())
        for _ in range(2):  # solid two samples around, so neither on a face nor next to one
            for axis in range(3):
                core = core & R._shift(core, 1, axis, False) & R._shift(core, -1, axis, False)
        d[~np.isfinite(d) | (~core if core.any() else False)] = np.inf
        x, z, y = np.unravel_index(int(np.argmin(d)), d.shape)
        r = 1.2
        self._brushes(slot, [v.sphere_brush(B.SUBTRACT, (float(x), float(y), float(z)), r, 0.0, 0.6, 0)])

    def stamp(self, dst, src):
        d, s, rng = self.m[dst], self.m[src], self.rng
        t = self.next_turn("stamp")
        c = (d.N - 1) / 2.0
        at = c + rng.uniform(-0.25, 0.25, 3) * (d.N - 1)
        scale = float(rng.uniform(0.4, 0.8)) * (d.N - 1) / (s.N - 1)
        rec = v.stamp_from_placement(s.N, tuple(at), quat((1.0, 2.0, 3.0), float(rng.uniform(10.0, 80.0))), scale, op=t % 3,
                                     blend=(0.0, 1.0)[t % 2], reach=2.0, material=(ST.KEEP, ST.SOURCE, 5)[(t // 3) % 3])
        new = d.copy()
        want = new.stamp(s, rec)
        self.step("stamp", dst, want, new, src=src, record=rec)

    def _region(self, slot, small: bool):
        """The keywords of a region: a ball of 3 cells on the solid's surface, or a box over the whole grid."""
        N = self.m[slot].N
        c = (N - 1) / 2.0
        if not small:
            return dict(shape=_abi.BRUSH_BOX, a=(c, c, c), b=(float(N), float(N), float(N)), radius=0.0)
        way = self.rng.standard_normal(3)
        way /= np.linalg.norm(way)
        return dict(shape=_abi.BRUSH_SPHERE, a=tuple(c + way * 0.3 * (N - 1)), b=(0.0, 0.0, 0.0), radius=3.0)

    def _scratch(self, kind, slot, region_mask) -> int:
        """Bytes of the shared scratch buffer the call needs, from the region's box: 12 per sample of the box grown by one for a
        smooth, 5 per sample of the box for a warp."""
        if not region_mask.any():
            return 0
        N = self.m[slot].N
        n = 1
        for idx in np.nonzero(region_mask):
            lo, hi = int(idx.min()), int(idx.max())
            if kind == "smooth":
                lo, hi = max(lo - 1, 0), min(hi + 1, N - 1)
            n *= hi - lo + 1
        return n * (12 if kind == "smooth" else 5)

    def smooth(self, slot, small: bool):
        t = self.next_turn("smooth")
        rec = v.smooth_record(strength=(0.5, 1.0, 0.25)[t % 3], iterations=(1, 2, 3)[t % 3], falloff=(2.0, 0.75)[t % 2],
                              rebound=(0.0, 0.0, 1.0)[t % 3], material=(-1, 7)[t % 2], **self._region(slot, small))
        new = self.m[slot].copy()
        scratch = self._scratch("smooth", slot, S.weights(rec, new.N)[0])
        want = new.smooth(rec)
        self.step("smooth", slot, want, new, record=rec, scratch=scratch)

    def warp(self, slot, small: bool):
        t = self.next_turn("warp")
        region = self._region(slot, small)
        N = self.m[slot].N
        c = np.asarray(region["a"], np.float64)
        motion = t % 4
        kw = {}
        if motion == 0:
            kw["pull"] = v.warp_from_motion((0.0, 0.0, 0.0), translation=(1.3, -0.6, 0.4))[0]
        elif motion == 1:
            kw["pull"] = v.warp_from_motion(tuple(c + (0.3, -0.2, 0.4)), rotation=quat((1.0, 2.0, 3.0), 23.0))[0]
            kw["strength"] = 0.7
        elif motion == 2:
            kw["pull"], kw["length_scale"] = v.warp_from_motion(tuple(c), scale=1.25)
        else:
            kw["inflate"] = (1.5, -0.7)[(t // 4) % 2]
        rec = v.warp_record(falloff=2.0 if small else 0.3 * N, material=(W.SOURCE, W.KEEP, 7)[(t // 2) % 3], **region, **kw)
        self._warp(slot, rec)

    def _warp(self, slot, rec):
        new = self.m[slot].copy()
        scratch = self._scratch("warp", slot, W.weights(rec, new.N)[0])
        want = new.warp(rec)
        self.step("warp", slot, want, new, record=rec, scratch=scratch)

    def warp_ids_only(self, slot):
        """A grab that takes the source's ids inside the box of zero_box: every density it moves is +0 and stays +0."""
        c = float((self.m[slot].N - 1) // 2)
        rec = v.warp_record(_abi.BRUSH_SPHERE, (c + 0.3, c, c - 0.2), (0.0, 0.0, 0.0), 2.5, falloff=1.0, material=W.SOURCE,
                            pull=v.warp_from_motion((0.0, 0.0, 0.0), translation=(1.0, 0.5, 0.0))[0])
        self._warp(slot, rec)

    def fill(self, slot):
        m = self.m[slot]
        new = m.copy()
        wall = float(np.float32(0.5) * m.unit)
        want = new.fill(wall, 1)
        self.step("fill", slot, want, new, wall=wall, material=1)

    def components(self, slot, op, refused: bool = False):
        m = self.m[slot]
        N = m.N
        kw = dict(op=op)
        if op != CR.REPORT:
            kw.update(gap=float(np.float32(0.5) * m.unit), material_id=(-1, 0)[self.next_turn("components") % 2])
        if op == CR.REMOVE_SMALL:
            kw["min_samples"] = 30
        solid = CR.solid(m.decoded())
        if op in (CR.KEEP_SEED, CR.REMOVE_SEED):
            if refused:
                near = solid.copy()
                for axis in range(3):
                    near = near | R._shift(near, 1, axis, False) | R._shift(near, -1, axis, False)
                free = np.argwhere(~near)
                x, z, y = free[int(self.rng.integers(len(free)))]
            elif op == CR.REMOVE_SEED:  # the smallest component: an island such as the -inf sample of analytic_field
                x, y, z = CR.component_list(CR.labels_of(solid))[-1]["first"]
            else:
                d = np.array(m.decoded(), np.float64)
                d[~np.isfinite(d)] = np.inf
                x, z, y = np.unravel_index(int(np.argmin(d)), d.shape)
            kw["seed"] = (int(x), int(y), int(z))
        new = m.copy()
        want = new.components(list_capacity=4, **kw)
        assert (want == REFUSED) == refused
        self.step("components", slot, want, new, list_capacity=4, **kw)

    def redistance(self, slot, whole: bool):
        m = self.m[slot]
        t = self.next_turn("redistance")
        band, from_ = BANDS[t % 3], FROMS[(t // 3 + t) % 3]
        lo = hi = None
        if not whole:
            last_lo, last_hi = self.last_box[slot]
            lo = tuple(max(a - band, 0) for a in last_lo)
            hi = tuple(min(a + band, m.N - 1) for a in last_hi)
        new = m.copy()
        want = new.redistance(band, from_, lo, hi)
        self.step("redistance", slot, want, new, band=band, from_=from_, lo=lo, hi=hi)

    # -- reads -------------------------------------------------------------------------------------------------------------------------
    def _box(self, slot):
        N, rng = self.m[slot].N, self.rng
        lo = [int(rng.integers(0, N - 2)) for _ in range(3)]
        hi = [int(rng.integers(l + 1, N)) for l in lo]
        return tuple(lo), tuple(hi)

    def extract_mesh(self, slot, whole: bool):
        lo, hi = (None, None) if whole else self._box(slot)
        iso = (0.0, float(np.float32(0.3) * self.m[slot].unit))[self.next_turn("extract_mesh") % 2]
        self.step("extract_mesh", slot, self.m[slot].extract_mesh(iso, lo, hi), iso=iso, lo=lo, hi=hi)

    def download_region(self, slot):
        lo, hi = self._box(slot)
        self.step("download_region", slot, self.m[slot].download_region(lo, hi), lo=lo, hi=hi)

    def download_volume(self, slot):
        self.step("download_volume", slot, self.m[slot].download_volume())


def _script(g: _Generator):
    """The calls of a program.  P is the slot that grows (17^3, later 33^3), Q the one that shrinks (33^3, then 5^3 or 9^3, then 17^3
    uploaded over it while it is in use)."""
    P = int(g.rng.integers(2))
    Q = 1 - P
    fp = g.formats[int(g.rng.integers(len(g.formats)))]
    fq = g.other_format(fp)
    g.upload(P, 4, fp)
    g.upload(Q, 5, fq)
    g.set_metric(P, True)
    g.set_metric(Q, True)
    g.brushes(P)
    g.update_region(Q, records=False)
    g.stamp(P, Q)                   # the source was edited by the step before
    g.smooth(P, small=True)
    g.warp(P, small=False)          # needs more of the shared scratch than any call before
    g.smooth(P, small=True)         # ... and this one less, directly after the other kind has left its layout there
    g.download_region(P)
    g.set_metric(P, False)
    g.brushes(P, outside=True)      # an edit while the tables are off
    g.zero_box(P)
    g.warp_ids_only(P)
    g.set_metric(P, True)           # the tables come back: the seeds must be whole
    g.cavity(P)
    g.fill(P)
    g.fill(P)                       # fills nothing
    g.redistance(P, whole=False)    # the fill's box grown by the band
    g.extract_mesh(P, whole=True)
    g.components(Q, CR.REPORT)
    g.components(Q, CR.KEEP_SEED, refused=True)
    g.components(Q, CR.REMOVE_SEED, refused=True)
    g.components(Q, CR.REMOVE_SMALL)
    g.download_volume(P)
    g.free(P)
    g.upload(P, 5, g.other_format(fp))  # grows, in the other format, from the metric (1, 0)
    g.smooth(P, small=False)        # more scratch than any call before
    g.warp(P, small=True)           # less, directly after a smooth
    g.set_metric(P, True)
    g.stamp(Q, P)
    g.redistance(Q, whole=False)
    g.free(Q)
    g.upload(Q, 2 + (g.seed + int(g.rng.integers(2))) % 2, g.other_format(fq))  # shrinks
    g.set_metric(Q, True)
    g.brushes(Q)
    g.warp(Q, small=False)
    g.upload(Q, 4, fq)              # over a slot in use: the metric stays
    g.components(P, (CR.KEEP_SEED, CR.REMOVE_SEED)[g.seed % 2])
    g.components(P, CR.KEEP_LARGEST)
    g.extract_mesh(Q, whole=False)
    g.download_volume(Q)
    g.update_region(Q, records=True)
    g.smooth(Q, small=True)
    g.redistance(Q, whole=True)
    g.download_region(Q)


N_STEPS = 47


@functools.lru_cache(maxsize=None)
def program(seed: int, n_steps: int = N_STEPS, formats=(R.F32, R.TEXEL16)):
    """The first n_steps steps of the seed's program: dicts {"n", "kind", "slot", "args", "want", "after"} — `want` is the record the
    call must report (the output, for a read-only call; None where the call reports nothing), `after` the two SlotModels after the
    step.  Computed once per (seed, n_steps, formats) and never written to afterwards."""
    g = _Generator(seed, formats)
    _script(g)
    assert len(g.steps) == N_STEPS and 1 <= n_steps <= N_STEPS
    return tuple(g.steps[:n_steps])


def coverage(steps) -> dict:
    """What the program reaches, counted from the model alone."""
    out = {"steps": len(steps), "kinds": {k: sum(s["kind"] == k for s in steps) for k in KINDS}}
    edits = [s for s in steps if s["kind"] in EDITS]
    out["edits"], out["edits_that_write"] = len(edits), sum(wrote(s["kind"], s["want"]) for s in edits)
    out["refused_twice_in_a_row"] = sum(a["want"] == REFUSED and b["want"] == REFUSED for a, b in zip(steps, steps[1:]))
    out["fills_of_nothing_after_a_fill"] = sum(a["kind"] == b["kind"] == "fill" and a["want"]["filled"] > 0 and b["want"]["filled"] == 0
                                               for a, b in zip(steps, steps[1:]))
    out["warps_of_ids_only"] = sum(s["kind"] == "warp" and s["want"]["written"] > 0 and s["want"]["density_writes"] == 0 for s in steps)
    most, last = 0, None
    for kind in ("smooth", "warp"):
        out[kind + "_grows_scratch"] = out[kind + "_fits_in_dirty_scratch"] = 0
    for s in steps:
        if s["kind"] not in ("smooth", "warp"):
            continue
        need = s["args"]["scratch"]
        if need > most and last is not None:
            out[s["kind"] + "_grows_scratch"] += 1
        if last is not None and last["kind"] != s["kind"] and 0 < need < last["args"]["scratch"]:
            out[s["kind"] + "_fits_in_dirty_scratch"] += 1
        most, last = max(most, need), s
    edited_off, back_on, edited = {}, 0, set()
    grows = shrinks = stamps_of_edited = kept_metric = fresh_metric = 0
    before = (SlotModel(), SlotModel())
    for s in steps:
        slot, was, now = s["slot"], before[s["slot"]], s["after"][s["slot"]]
        if s["kind"] in EDITS and wrote(s["kind"], s["want"]):
            edited.add(slot)
            if not was.tables:
                edited_off[slot] = True
        if s["kind"] == "set_metric" and now.tables and edited_off.pop(slot, False):
            back_on += 1
        if s["kind"] == "stamp" and s["args"]["src"] in edited:
            stamps_of_edited += 1
        if s["kind"] == "upload":
            edited.discard(slot)
            edited_off.pop(slot, None)
            sized = [p["after"][slot].N for p in steps[:s["n"]] if p["slot"] == slot and p["after"][slot].used]
            if sized:
                grows += now.N > sized[-1]
                shrinks += now.N < sized[-1]
            kept_metric += was.used and (was.scale, was.step) != (1.0, 0.0)
            fresh_metric += (not was.used) and any(p["slot"] == slot and p["after"][slot].used and
                                                   (p["after"][slot].scale, p["after"][slot].step) != (1.0, 0.0) for p in steps[:s["n"]])
        before = s["after"]
    out.update(edits_with_tables_off_then_on=back_on, uploads_that_grow=grows, uploads_that_shrink=shrinks,
               stamps_of_an_edited_source=stamps_of_edited, uploads_that_keep_a_metric=kept_metric, uploads_after_a_free_of_a_metric=fresh_metric)
    out["slots_with_a_surface_at_the_end"] = sum(m.used and bool(CR.solid(m.decoded()).any()) and not CR.solid(m.decoded()).all()
                                                 for m in steps[-1]["after"])
    out["resolutions"] = sorted({s["args"]["res"] for s in steps if s["kind"] == "upload"})
    out["upload_paths"] = sorted({s["args"]["path"] for s in steps if s["kind"] == "upload"})
    return out


def shortfalls(cov: dict) -> list:
    """The conditions of a program that a coverage count misses (none, for a seed the tests may use)."""
    bad = [f"{k} occurs {n} times" for k, n in cov["kinds"].items() if n < 2]
    if cov["edits_that_write"] < 0.7 * cov["edits"]:
        bad.append(f"only {cov['edits_that_write']} of {cov['edits']} edits write")
    if cov["edits_that_write"] == cov["edits"]:
        bad.append("no edit is a no-op")
    for key in ("smooth_grows_scratch", "warp_grows_scratch", "smooth_fits_in_dirty_scratch", "warp_fits_in_dirty_scratch",
                "edits_with_tables_off_then_on", "uploads_that_grow", "uploads_that_shrink", "stamps_of_an_edited_source",
                "uploads_that_keep_a_metric", "uploads_after_a_free_of_a_metric", "refused_twice_in_a_row", "fills_of_nothing_after_a_fill",
                "warps_of_ids_only"):
        if cov[key] < 1:
            bad.append(f"{key} is {cov[key]}")
    if cov["slots_with_a_surface_at_the_end"] < len(SLOTS):
        bad.append("a slot ends without a surface")
    return bad
