"""The placed pairs of volumes the contact tests run, on the host (test_query_contacts.py) and on the device (test_query_contacts_gpu.py):
two sphere fields of extent 1 whose centres lie off the grid, A at the origin and B turned by a general quaternion, so that the spheres
overlap by a given part of a cell of A; and the pairs the header's corner cases name.  A Side is one placed volume as a test hands it to
contacts_ref (slot / inst), to the host pass (stored / placed) and to the renderer (volume / placement)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence

import numpy as np

import points_ref as P
from volume_ref import F32, TEXEL16, dense_field

f32 = np.float32
RADIUS = {9: 2.6, 17: 5.3, 33: 10.4, 65: 20.7, 129: 20.7}  # N: the sphere's radius in cells
QUAT = (0.18257418, 0.36514837, 0.54772256, 0.73029674)     # (1, 2, 3, 4) / sqrt(30): a general rotation
TEXEL_GAIN = 8.0  # a TEXEL16 side stores its distance in eighths of a cell, so that a texel is 1 / 800 of a cell


@dataclass
class Side:
    density: np.ndarray                 # float32 [x, z, y]: what is uploaded
    material: np.ndarray                # uint8 [x, z, y]
    fmt: int = F32
    extent: float = 1.0
    density_scale: float = 1.0
    step_max: float = 0.0
    position: Sequence[float] = (0.0, 0.0, 0.0)
    rotation: Sequence[float] = (0.0, 0.0, 0.0, 1.0)
    scale: Sequence[float] = (1.0, 1.0, 1.0)
    centre: Sequence[float] = field(default=(0.0, 0.0, 0.0))  # of the sphere, object space
    radius: float = 0.0                                        # object units

    @property
    def N(self) -> int:
        return self.density.shape[0]

    @property
    def stored(self) -> np.ndarray:
        return dense_field(self.density, self.fmt)

    def slot(self) -> P.Slot:
        return P.Slot(self.stored, self.material, self.fmt, self.extent, self.density_scale, self.step_max)

    def inst(self) -> P.Instance:
        return P.Instance(0, tuple(self.position), tuple(self.rotation), tuple(self.scale))

    def placed(self) -> dict:
        return {"extent": self.extent, "texel16": self.fmt == TEXEL16, "density_scale": self.density_scale, "step_max": self.step_max,
                "position": self.position, "rotation": self.rotation, "scale": self.scale}

    def world_centre(self) -> np.ndarray:
        W = P.pack_w2o(self.rotation, (1.0, 1.0, 1.0)).astype(np.float64)  # R^T; object -> world is S R
        return np.asarray(self.scale, np.float64) * (W.T @ np.asarray(self.centre, np.float64)) + np.asarray(self.position, np.float64)


def sphere(N: int, fmt: int = F32, radius_cells: float = None, centre=(0.013, -0.021, 0.017), seed: int = 1, **placement) -> Side:
    """A sphere's signed distance on an N^3 grid of extent 1 — in object units with density_scale 1 (F32), or in eighths of a cell with
    the density_scale that takes them back (TEXEL16) —, seeded material ids."""
    cell = 2.0 / (N - 1)
    r = (RADIUS[N] if radius_cells is None else radius_cells) * cell
    a = (np.arange(N, dtype=np.float64) * cell - 1.0)
    X, Z, Y = a[:, None, None], a[None, :, None], a[None, None, :]
    d = np.sqrt((X - centre[0]) ** 2 + (Y - centre[1]) ** 2 + (Z - centre[2]) ** 2) - r
    material = np.random.default_rng(seed + N).integers(1, 256, (N, N, N)).astype(np.uint8)
    if fmt == TEXEL16:
        unit = cell / TEXEL_GAIN
        return Side((d / unit).astype(f32), material, fmt, density_scale=float(f32(unit)), centre=centre, radius=r, **placement)
    return Side(d.astype(f32), material, fmt, centre=centre, radius=r, **placement)


def rest_on(a: Side, b: Side, overlap_cells: float, direction=(1.0, 0.4, -0.3)) -> Side:
    """b moved so that its sphere's world centre lies along `direction` from a's, the two spheres (as a's and b's smallest scales make
    them) overlapping by overlap_cells cells of a."""
    u = np.asarray(direction, np.float64)
    u /= np.linalg.norm(u)
    ra = a.radius * min(abs(s) for s in a.scale)
    rb = b.radius * min(abs(s) for s in b.scale)
    gap = ra + rb - overlap_cells * 2.0 * a.extent / (a.N - 1)
    b.position = (0.0, 0.0, 0.0)
    shift = a.world_centre() + u * gap - b.world_centre()
    b.position = tuple(float(f32(x)) for x in shift)
    return b


def pair(na: int, nb: int, overlap: float, fmt_a: int = F32, fmt_b: int = F32, a_kw=None, b_kw=None, direction=(1.0, 0.4, -0.3)):
    a = sphere(na, fmt_a, seed=1, **(a_kw or {}))
    b = sphere(nb, fmt_b, centre=(-0.011, 0.019, 0.023), seed=2, **({"rotation": QUAT} | (b_kw or {})))
    return a, rest_on(a, b, overlap, direction)


def nan_in_b():
    """The 17^3 pair with every sample of B's half towards A made NaN around the contact: those cells give no candidate."""
    a, b = pair(17, 17, 1.0)
    w = P.pack_w2o(b.rotation, b.scale).astype(np.float64) @ (a.world_centre() - np.asarray(b.position, np.float64))  # A's centre in B's object space
    g = np.clip(np.round((w / np.linalg.norm(w) * b.radius + 1.0) * 8.0).astype(int), 1, 15)  # the grid point of B's surface nearest A
    b.density = b.density.copy()
    b.density[g[0] - 1:g[0] + 1, g[2] - 1:g[2] + 1, g[1] - 1:g[1] + 1] = np.nan
    return a, b


def disjoint():
    a, b = pair(9, 9, 1.0)
    b.position = (5.0, 0.25, -0.5)
    return a, b


def corner_only():
    """A's surface (a sphere larger than its box leaves it near the corners) under a small B whose box covers one corner of A only."""
    a = sphere(17, radius_cells=12.0)  # radius 1.5: the corners lie at 1.73
    b = sphere(9, centre=(-0.011, 0.019, 0.023), seed=2, rotation=QUAT, scale=(0.4, 0.4, 0.4))
    u = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    b.position = tuple(float(f32(x)) for x in a.world_centre() + u * (a.radius + 0.15) - (b.world_centre() - np.asarray(b.position)))
    return a, b


def b_contains_a(na: int = 9):
    """B's box and B's solid both hold all of A: every vertex of A is a candidate and a contact."""
    a = sphere(na)
    b = sphere(9, centre=(-0.011, 0.019, 0.023), seed=2, rotation=QUAT, scale=(3.0, 3.0, 3.0), position=(0.05, -0.1, 0.07))
    return a, b


CASES = {
    "spheres9_overlap1": lambda: pair(9, 9, 1.0),
    "spheres9_overlap025": lambda: pair(9, 9, 0.25),
    "spheres17_overlap1": lambda: pair(17, 17, 1.0),
    "spheres17_overlap025": lambda: pair(17, 17, 0.25),
    "texel16_a": lambda: pair(17, 17, 1.0, TEXEL16, F32),
    "texel16_b": lambda: pair(17, 17, 1.0, F32, TEXEL16),
    "texel16_both": lambda: pair(17, 17, 1.0, TEXEL16, TEXEL16),
    "b_scaled_rotated": lambda: pair(17, 17, 1.0, b_kw={"scale": (1.2, 0.8, 1.1)}),
    "a_scaled_rotated": lambda: pair(17, 17, 1.0, a_kw={"scale": (0.9, 1.3, -1.1), "rotation": (0.5, -0.5, 0.5, 0.5), "position": (0.3, -0.2, 0.1)}),
    "step_max_and_scale": lambda: pair(17, 17, 1.0, b_kw={"scale": (2.0, 2.0, 2.0), "step_max": 0.05}),
    "a33_b9": lambda: pair(33, 9, 1.0),
    "nan_in_b": nan_in_b,
    "disjoint": disjoint,
    "corner_only": corner_only,
    "b_contains_a": b_contains_a,
}
EMPTY = ("disjoint",)  # no candidate at all


def margins(a: Side):
    """0, and half a cell of A."""
    return (0.0, float(f32(0.5 * 2.0 * a.extent / (a.N - 1))))
