"""The cases of the mask tests, shared by the host pass (tests/test_volume_mask.py) and the device (tests/test_volume_mask_gpu.py): for
a grid size N a list of (name, records), each applied to a slot without a mask that holds extreme_cases.small_field(N, fmt), and the
reference's answer, computed once per (N, fmt).  The sizes: single-word rows (N <= 33), the smallest grid with a second word per row,
which holds one live bit (N = 65), and three words (N = 129)."""
from __future__ import annotations

import functools

import numpy as np

import extreme_cases as X
import mask_ref as MK
from mask_ref import ALL, GROW, INVERT, MATERIAL, SHAPE, SHRINK, SOLID, op
from volumetricraytracer_amd import _abi

SIZES = (2, 3, 5, 9, 33, 65, 129)
SPHERE, BOX, CAPSULE = _abi.BRUSH_SPHERE, _abi.BRUSH_BOX, _abi.BRUSH_CAPSULE


def slab(N: int, y0: int, y1: int, value: int = 1):
    """A BOX record over every x and z and the samples y0..y1."""
    c = (N - 1) / 2.0
    return op(SHAPE, value, BOX, a=(c, (y0 + y1) / 2.0, c), b=(float(N), (y1 - y0) / 2.0 + 0.25, float(N)))


def cases(N: int):
    c = (N - 1) / 2.0
    off = (c + 0.3, c - 0.2, c + 0.1)  # off the lattice
    r = 0.3 * (N - 1) + 0.6
    ball = op(SHAPE, 1, SPHERE, a=off, radius=r)
    out = [
        ("all", [op(ALL, 1)]),
        ("a shrink of all leaves all", [op(ALL, 1), op(SHRINK, steps=3)]),
        ("an invert of nothing is all", [op(INVERT)]),
        ("all, released again", [op(ALL, 1), op(ALL, 0)]),
        ("sphere", [ball]),
        ("box with rounded edges, across a face", [op(SHAPE, 1, BOX, a=(N - 1.0, c, c + 0.4), b=(r, 0.5 * r, 0.7 * r), radius=0.2 * r)]),
        ("capsule", [op(SHAPE, 1, CAPSULE, a=(0.0, 0.2, c), b=(N - 1.0, N - 1.3, c), radius=0.15 * N + 0.5)]),
        ("all but a sphere", [op(ALL, 1), op(SHAPE, 0, SPHERE, a=off, radius=r)]),
        ("a shape outside the grid", [op(ALL, 1), op(SHAPE, 0, SPHERE, a=(-5.0 * N, c, c), radius=1.0)]),
        ("material 17", [op(MATERIAL, 1, material=17)]),
        ("solid", [op(SOLID, 1)]),
        ("solid, inverted, a material released", [op(SOLID, 1), op(INVERT), op(MATERIAL, 0, material=32)]),
        ("sphere grown by 2", [ball, op(GROW, steps=2)]),
        ("sphere shrunk by 1", [ball, op(SHRINK, steps=1)]),
        ("a sample grown to every face", [op(SHAPE, 1, SPHERE, a=(float(N // 2),) * 3, radius=0.25), op(GROW, steps=max(1, N // 2))]),
        ("shrink does not eat from the faces", [slab(N, 0, N // 2), op(SHRINK, steps=2)]),
        ("a sequence", [op(SOLID, 1), op(GROW, steps=1), ball, op(INVERT), op(SHRINK, steps=1), op(MATERIAL, 1, material=33),
                        op(SHAPE, 0, BOX, a=off, b=(0.2 * N + 0.5,) * 3, radius=0.0), op(GROW, steps=3)]),
    ]
    if N >= 65:  # fronts across y = 63 | 64, the boundary of the row's first two words, from either side
        out += [
            ("grow up across 63|64", [slab(N, 60, 62), op(GROW, steps=3)]),
            ("grow down across 63|64", [slab(N, 64, 64), op(GROW, steps=2)]),
            ("shrink up across 63|64", [op(ALL, 1), slab(N, 60, 62, 0), op(SHRINK, steps=3)]),
            ("shrink down across 63|64", [op(ALL, 1), slab(N, 64, 64, 0), op(SHRINK, steps=2)]),
        ]
    return out


@functools.lru_cache(maxsize=None)
def reference(N: int, fmt: int):
    """{name: the mask the case leaves}, read-only."""
    stored, material = X.small_field(N, fmt)
    out = {}
    for name, ops in cases(N):
        out[name] = MK.apply(None, ops, stored, material, fmt)
        out[name].setflags(write=False)
    return out


def check_cases_are_what_they_say(N: int, ref: dict):
    """From the reference alone: the cases reach what the tests are for."""
    full = N ** 3
    assert ref["all"].all() and ref["a shrink of all leaves all"].all() and ref["an invert of nothing is all"].all()
    assert not ref["all, released again"].any()
    assert int(ref["a shape outside the grid"].sum()) == full
    grown = ref["a sample grown to every face"]
    assert all(grown.take(i, axis).any() for axis in range(3) for i in (0, N - 1))
    eaten = ref["shrink does not eat from the faces"]
    assert N < 5 or (eaten[:, :, 0].all() and not eaten.all())
    if N >= 5:  # the ids of extreme_cases.small_field are (d <= 0) | (index % 5) << 4: 17, 32 and 33 are among them
        for name in ("sphere", "capsule", "solid", "material 17", "a sequence", "sphere shrunk by 1"):
            assert 0 < int(ref[name].sum()) < full, name
        assert int(ref["sphere grown by 2"].sum()) > int(ref["sphere"].sum()) > int(ref["sphere shrunk by 1"].sum())
    if N >= 65:
        up, down = ref["grow up across 63|64"], ref["grow down across 63|64"]
        assert up[0, 0, 57:66].all() and not up[0, 0, 66:].any() and not up[0, 0, :57].any()
        assert down[0, 0, 62:min(67, N)].all() and not down[0, 0, :62].any()
        up, down = ref["shrink up across 63|64"], ref["shrink down across 63|64"]
        assert not up[0, 0, 57:66].any() and up[0, 0, :57].all() and up[0, 0, 66:].all()
        assert not down[0, 0, 62:min(67, N)].any() and down[0, 0, :62].all()


def refused_records():
    """(what is wrong, records) — each refused with VRT_ERR_INVALID; every other field is acceptable."""
    nan, inf = float("nan"), float("inf")
    good = op(SHAPE, 1, SPHERE, a=(1.0, 1.0, 1.0), radius=1.0)

    def reserved(i):
        r = op(ALL, 1)
        r.reserved_[i] = 1
        return r

    bad = [
        ("kind -1", [op(-1)]), ("kind 7", [op(7)]),
        ("value 2", [op(ALL, 2)]), ("value -1", [op(SOLID, -1)]),
        ("value on INVERT", [op(INVERT, 1)]), ("value on GROW", [op(GROW, 1, steps=1)]), ("value on SHRINK", [op(SHRINK, 1, steps=1)]),
        ("shape 3", [op(SHAPE, 1, 3, a=(1.0, 1.0, 1.0), radius=1.0)]), ("shape -1", [op(SHAPE, 1, -1, radius=1.0)]),
        ("NaN centre", [op(SHAPE, 1, SPHERE, a=(nan, 1.0, 1.0), radius=1.0)]),
        ("infinite b", [op(SHAPE, 1, SPHERE, a=(1.0, 1.0, 1.0), b=(0.0, inf, 0.0), radius=1.0)]),
        ("NaN radius", [op(SHAPE, 1, SPHERE, radius=nan)]),
        ("sphere radius 0", [op(SHAPE, 1, SPHERE, radius=0.0)]), ("capsule radius -1", [op(SHAPE, 0, CAPSULE, b=(1.0, 0.0, 0.0), radius=-1.0)]),
        ("box half size 0", [op(SHAPE, 1, BOX, b=(1.0, 0.0, 1.0))]), ("box radius -1", [op(SHAPE, 1, BOX, b=(1.0, 1.0, 1.0), radius=-1.0)]),
        ("capsule a == b", [op(SHAPE, 1, CAPSULE, a=(1.0, 2.0, 3.0), b=(1.0, 2.0, 3.0), radius=1.0)]),
        ("material -1", [op(MATERIAL, 1, material=-1)]), ("material 256", [op(MATERIAL, 0, material=256)]),
        ("grow steps 0", [op(GROW, steps=0)]), ("shrink steps 65", [op(SHRINK, steps=_abi.MAX_MASK_STEPS + 1)]),
        ("grow steps -1", [op(GROW, steps=-1)]),
        ("a bad record after good ones", [good, op(INVERT), op(GROW, steps=0)]),
        ("33 records", [op(INVERT)] * (_abi.MAX_MASK_OPS + 1)),
    ]
    bad += [(f"reserved word {i}", [reserved(i)]) for i in range(4)]
    return bad


def accepted_records():
    """Records at the edges of the rules, each accepted."""
    return [[], [op(INVERT)] * _abi.MAX_MASK_OPS, [op(GROW, steps=_abi.MAX_MASK_STEPS)], [op(MATERIAL, 1, material=255)],
            [op(SHAPE, 0, BOX, b=(1.0, 1.0, 1.0), radius=0.0)], [op(INVERT, material=-7, steps=99, shape=12)]]


# ---- honouring edit calls, over the session model ------------------------------------------------------------------------------------

HONOURING = ("brushes", "stamp", "smooth", "warp", "fill", "components", "redistance")


def z_half(N: int, value: int = 1):
    """A BOX record over the samples with z < N // 2."""
    c = (N - 1) / 2.0
    return op(SHAPE, value, BOX, a=(c, c, 0.0), b=(float(N), float(N), N // 2 - 0.5))


def honour(g, masks: dict, slot: int, edit):
    """Runs a generator's edit (which appends its step and leaves the slot's model as the unmasked call leaves it), then puts the
    protected samples back: the step's `after` and the generator's model carry the masked state on; the step's `want` stays the
    unmasked run's record.  The step gains "restored" and "unprotected" (how many unprotected samples changed)."""
    before = g.m[slot]
    edit()
    step, after = g.steps[-1], g.m[slot]
    assert step["slot"] == slot and step["kind"] in HONOURING
    mask = masks.get(slot)
    if mask is None:
        mask = np.zeros(before.stored.shape, bool)
    stored, material, restored = MK.protect(mask, before.stored, before.material, after.stored, after.material)
    new = after.copy()
    new._set(stored, material)
    g.m[slot] = new
    step["after"] = tuple(g.m)
    step["restored"] = restored
    step["unprotected"] = int(((MK.bits(before.stored) != MK.bits(stored)) | (before.material != material)).sum())
    return step


def mask_step(g, masks: dict, slot: int, ops):
    """A vrt_volume_mask_apply step: the reference's mask for the slot, carried in `masks`."""
    m = g.m[slot]
    masks[slot] = MK.apply(masks.get(slot), ops, m.stored, m.material, m.fmt)
    masks[slot].setflags(write=False)
    g.steps.append({"kind": "mask", "slot": slot, "args": {"ops": ops}, "want": MK.info(masks[slot]), "after": tuple(g.m), "n": len(g.steps),
                    "mask": masks[slot]})
    return g.steps[-1]


def _edit_of(g, kind: str):
    import components_ref as CR
    return {"brushes": lambda: g.brushes(0), "stamp": lambda: g.stamp(0, 1), "smooth": lambda: g.smooth(0, small=False),
            "warp": lambda: g.warp(0, small=False), "fill": lambda: g.fill(0), "components": lambda: g.components(0, CR.REMOVE_SMALL),
            "redistance": lambda: g.redistance(0, whole=True)}[kind]


@functools.lru_cache(maxsize=None)
def edit_case(kind: str, fmt: int, res: int = 5):
    """One honouring call on a freshly uploaded slot 0 with the tables on and the half z < N / 2 protected (slot 1 holds the stamp's 5^3
    source): the steps, the last of which is the edit with its masked `after`."""
    import session_model as M
    g = M._Generator(70 + res, (fmt,))
    N = (1 << res) + 1
    g.upload(1, 2, fmt)
    if kind == "fill":  # solid with the samples that lie on no face hollow
        sealed = X.fill_fields(N)["sealed"][0]
        args = dict(res=res, extent=M.EXTENTS[0], fmt=fmt, path="float", density=M._frozen(sealed, np.float32),
                    material=M._frozen(np.zeros((N, N, N), np.uint8), np.uint8))
        new = g.m[0].copy()
        new.upload(**args)
        g.step("upload", 0, None, new, **args)
    else:
        g.upload(0, res, fmt)
    g.set_metric(0, True)
    masks = {}
    mask_step(g, masks, 0, [z_half(N)])
    honour(g, masks, 0, _edit_of(g, kind))
    return tuple(g.steps)


def sequence(fp: int, fq: int):
    """Mask records and honouring edits alternating on two slots of different formats and sizes, with carried state: 16 such steps
    after the uploads."""
    import components_ref as CR
    import session_model as M
    g = M._Generator(91, (fp, fq))
    P, Q = 0, 1
    g.upload(P, 4, fp)
    g.upload(Q, 3, fq)
    g.set_metric(P, True)
    g.set_metric(Q, True)
    NP, NQ = g.m[P].N, g.m[Q].N
    cp, cq = (NP - 1) / 2.0, (NQ - 1) / 2.0
    masks = {}
    mask_step(g, masks, P, [op(SHAPE, 1, SPHERE, a=(cp + 3.3, cp, cp - 0.4), radius=6.5)])
    honour(g, masks, P, lambda: g.brushes(P))
    mask_step(g, masks, Q, [op(SOLID, 1)])
    honour(g, masks, Q, lambda: g.brushes(Q))
    mask_step(g, masks, P, [op(GROW, steps=2)])
    honour(g, masks, P, lambda: g.smooth(P, small=False))
    mask_step(g, masks, Q, [op(INVERT)])
    honour(g, masks, Q, lambda: g.stamp(Q, P))  # the source's mask is ignored
    mask_step(g, masks, P, [op(MATERIAL, 0, material=2), op(SHAPE, 1, CAPSULE, a=(0.0, cp, cp), b=(NP - 1.0, cp + 2.0, cp), radius=2.5)])
    honour(g, masks, P, lambda: g.warp(P, small=False))
    mask_step(g, masks, Q, [op(SHRINK, steps=1), z_half(NQ)])
    honour(g, masks, Q, lambda: g.redistance(Q, whole=True))
    mask_step(g, masks, P, [op(INVERT)])
    honour(g, masks, P, lambda: g.components(P, CR.REMOVE_SMALL))
    mask_step(g, masks, Q, [op(ALL, 0)])  # a mask without a set bit
    honour(g, masks, Q, lambda: g.brushes(Q))
    return tuple(g.steps)
