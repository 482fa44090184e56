"""Launch-level cases of pf_dccl_lookup_feat (csrc/pf_lookup.hip: pf_lookup_feat_kernel) at ragged maps and every channel layout
(not a conftest, nothing here is collected).  The same cases run on the CPU against the host emulation of pf_lookup_feat_elem
(tests/test_alt_corr_launch_reference.py) and on the GPU against the HIP library (tests/test_hip_alt_corr_launches.py), each
against the float64 restatement and the derived bound of tests/alt_corr_ref.py.

What a case is for
  maps      (1, 16, 16) the smallest the entry point takes; (3, 17, 27) odd at every level, a dead tile row and one dead wave per
            tile of the last tile column; (2, 18, 21) three dead waves there; (1, 16, 34) two; (1, 20, 45) the other ragged golden map.
  channels  4 and 36 (lanes without channels on the pixel path; a one-piece and a ragged last chunk on the tile path), 128, 256,
            260 (one lane with a second channel group, a 4-channel last chunk) and 512.  All of them on (3, 17, 27), 256 elsewhere.
  families  zero / nasty / large as tests/test_hip_alt_corr.py draws them, and `outside`: y at least 64 rows off the map, so no
            own-view corner of any tile carries a weight (nwin == 0: the tile path with no corner; the view must be exactly 0.0).
  stretch   x = sx * px + 0.5, y = sy * py + 0.5 on (1, 32, 64) with a cross-view grid that is constant at GRID_POINT: the family
            the path decision is pinned on, see `pin`.

Per launch: both outputs, every row and all 324 columns against float64 under alt_corr_ref.bound; ld = 336 with the 12 padding
columns prefilled with SENT_F32 and required untouched; the 324 live columns prefilled with NaN, so a row a live wave did not
write fails; a second launch bitwise equal; every image of a B > 1 launch bitwise equal to the B = 1 launch of that image.
"""
import math
from collections import OrderedDict

import torch

import alt_corr_ref as ref
import elem_launches as el
import golden_cases as gc
import priorflow_oracle as po

SENT_F32 = el.SENT_F32
CORR_CH, LD = 324, 336
MAPS = OrderedDict([("16x16", (1, 16, 16)), ("17x27", (3, 17, 27)), ("18x21", (2, 18, 21)), ("16x34", (1, 16, 34)),
                    ("20x45", (1, 20, 45))])
CHANNELS = (4, 36, 128, 256, 260, 512)
FAMILIES = ("zero", "nasty", "large", "outside")
CASES = [(C, "17x27", f) for C in CHANNELS for f in FAMILIES] + \
        [(256, m, f) for m in MAPS if m != "17x27" for f in FAMILIES]
STRETCH_MAP, STRETCH_C = (1, 32, 64), 256
STRETCH = ((1, 1), (2, 2), (2, 3))
GRID_POINT = (20.5, 11.5)            # interior of the 32 x 64 map and of every level the cross view reaches with it
STRETCH_CASES = [(STRETCH_C, "32x64", f"stretch{sx}x{sy}") for sx, sy in STRETCH]


def n_units(B, h, w):
    """(tile, level, view) units of one launch."""
    return B * ((h + ref.LF_TY - 1) // ref.LF_TY) * ((w + ref.LF_TX - 1) // ref.LF_TX) * 4 * 2


def _identity(B, h, w):
    return po.coords_grid(B, h, w).contiguous()


def coords_of(family, tag, B, h, w):
    c0 = _identity(B, h, w)
    if family == "zero":
        return c0
    if family == "nasty":
        return gc.nasty_coords(tag, B, h, w)
    if family == "large":
        return (c0 + gc.uni(tag + "/large", (B, 2, h, w), -40.0, 40.0)).contiguous()
    if family == "outside":          # x as scattered as `nasty`; y below the map on even columns, above it on odd ones
        co = c0 + gc.uni(tag + "/outside", (B, 2, h, w), -6.0, 6.0)
        off = gc.uni(tag + "/outside/y", (B, h, w), 0.0, 8.0)
        down = (torch.arange(w) % 2 == 0).view(1, 1, w)
        co[:, 1] = torch.where(down, h + 63.0 + off, -64.0 - off)
        assert bool(((co[:, 1] >= h + 63.0) | (co[:, 1] <= -64.0)).all())
        return co.contiguous()
    if family.startswith("stretch"):
        sx, sy = (int(v) for v in family[len("stretch"):].split("x"))
        return torch.stack([sx * c0[:, 0] + 0.5, sy * c0[:, 1] + 0.5], 1).contiguous()
    raise KeyError(family)


def make_case(C, map_name, family):
    B, h, w = STRETCH_MAP if map_name == "32x64" else MAPS[map_name]
    tag = f"altcorr/launch/{map_name}/{C}"
    c = dict(C=C, map=map_name, family=family, B=B, h=h, w=w)
    # gc.fmaps is fixed at 256 channels: the same range from the same generator
    for k in ("f1a", "f2a", "f1b", "f2b"):
        c[k] = gc.uni(f"{tag}/{k}", (B, C, h, w), -1.7, 1.7)
    c["coords"] = coords_of(family, f"{tag}/{family}", B, h, w)
    if family.startswith("stretch"):
        c["g"] = torch.stack([torch.full((h, w), GRID_POINT[0]), torch.full((h, w), GRID_POINT[1])]).contiguous()
    else:
        c["g"] = po.sample_grid(h, w, po.rotation_x(math.pi / 2)).contiguous()
    return c


def image_of(c, b):
    """The B = 1 case of image b."""
    one = dict(c, B=1)
    for k in ("f1a", "f2a", "f1b", "f2b", "coords"):
        one[k] = c[k][b:b + 1].contiguous()
    return one


def reference(c):
    """own / raw: (float64 value, bound), computed once per case."""
    args = (c["coords"], c["f1a"], c["f2a"], c["f1b"], c["f2b"], c["g"])
    w_own, w_raw = ref.lookup_feat(*args)
    m_own, m_raw = ref.lookup_feat(*args, absolute=True)
    return dict(own=(w_own, ref.bound(c["C"], m_own)), raw=(w_raw, ref.bound(c["C"], m_raw)))


# ------------------------------------------------------------------------------------------------------------------------
# the path decision, pinned
# ------------------------------------------------------------------------------------------------------------------------
def immune(p):
    """A position whose floor cannot differ between two fp32 evaluations of the same formula: exactly 0 (all taps of the grid
    sample out of range), or a fractional part in [1/16, 15/16]."""
    f = p - torch.floor(p)
    return (p == 0) | ((f >= 1.0 / 16) & (f <= 15.0 / 16))


def pin(c):
    """The predicted path counts of a launch and whether they may be asserted exactly.

    A unit is IMMUNE when every position of its 8 x 81 taps is `immune`: own-view taps; for the cross view the grid taps and the
    position the grid sample returns.  The own view and the grid taps of the stretch family are multiples of 1/16 with an odd
    numerator at every level, immune everywhere.  The constant grid is not at the map border: where a grid tap hangs over the
    first row (or the last column before the seam) the sample returns GRID_POINT times the weight inside, (2m + 1) a / 32 for a
    weight a / 16, and for every half-integer m + 1/2 one odd a in 1 .. 15 lands on 1/32 or 31/32 (a (2m + 1) = +-1 mod 32) --
    level 3 meets every a.  So the prediction is masked: for a unit that is not immune the window is bracketed instead,
      lo = the box of the corners of its immune taps alone (a box only grows),
      hi = the box of all its corners and, for every tap that is not immune, of the whole 4 x 4 cell neighbourhood
           [floor - 1, floor + 2]^2 of the returned position inside the map (a floor one off in either direction, any weight),
    and the unit is DECIDED when hi <= LF_CAP or lo > LF_CAP.  (A unit whose GRID taps are not immune is never decided.)  The
    exact comparison is made only for launches in which every unit is immune or decided -- all three of the sweep, asserted by
    `stretch_sweep`; the masked units hold 4 .. 112 window rows there, nowhere near the cap."""
    B, h, w = c["B"], c["h"], c["w"]
    corn = ref.corners(c["coords"], c["g"])
    nwin, counts = ref.units(corn, B, h, w)
    tile, T = ref.tile_of_pixel(B, h, w)
    P = B * h * w
    imm = torch.zeros(T, 4, 2, dtype=torch.bool)
    decided = torch.zeros(T, 4, 2, dtype=torch.bool)
    for i, lv in enumerate(corn):
        Hl, Wl = h >> i, w >> i
        pos = lv["pos"]
        grid_ok = immune(pos["grid"][0]) & immune(pos["grid"][1])
        tap_ok = (immune(pos["own"][0]) & immune(pos["own"][1]), grid_ok & immune(pos["raw"][0]) & immune(pos["raw"][1]))
        for v, key in enumerate(("own", "raw")):
            ok = tap_ok[v]                                                         # [P, 81]
            bad_units = torch.zeros(T, dtype=torch.long).scatter_add(0, tile, (~ok).sum(1))
            imm[:, i, v] = bad_units == 0
            idx = lv[key][0]
            lo = ref.tile_boxes(torch.where(ok[..., None], idx, torch.full_like(idx, -1)).reshape(P, -1), Wl, tile, T)[1]
            x, y = pos[key]
            fx, fy = torch.floor(po._roundtrip(x, Wl)), torch.floor(po._roundtrip(y, Hl))
            extra = []
            for dy in (-1, 0, 1, 2):
                for dx in (-1, 0, 1, 2):
                    xi, yi = fx + dx, fy + dy
                    inside = (xi >= 0) & (xi <= Wl - 1) & (yi >= 0) & (yi <= Hl - 1) & ~ok
                    e = (yi.clamp(0, Hl - 1) * Wl + xi.clamp(0, Wl - 1)).long()
                    extra.append(torch.where(inside, e, torch.full_like(e, -1)))
            hi = ref.tile_boxes(torch.cat([idx.reshape(P, -1), torch.stack(extra, -1).reshape(P, -1)], 1), Wl, tile, T)[1]
            if v == 1:
                wild = torch.zeros(T, dtype=torch.long).scatter_add(0, tile, (~grid_ok).sum(1)) > 0
                hi = torch.where(wild, torch.full_like(hi, 1 << 40), hi)
            assert bool((lo <= nwin[:, i, v]).all()) and bool((nwin[:, i, v] <= hi).all())
            decided[:, i, v] = (hi <= ref.LF_CAP) | (lo > ref.LF_CAP)
    return dict(nwin=nwin, counts=counts, immune=imm, exact=bool((imm | decided).all()),
                masked=int((~imm).sum()), masked_nwin=sorted(set(nwin[~imm].tolist())))


def stretch_sweep():
    """[(case, pin)] of the sweep, with the conditions that make it worth running asserted on the CPU."""
    out = [(c, pin(c)) for c in (make_case(*k) for k in STRETCH_CASES)]
    for c, p in out:
        assert p["exact"], (c["family"], "a unit is neither immune nor decided")
        assert bool(p["immune"][:, :, 0].all()) and bool(p["immune"][:, :2, 1].all()), "own view / cross levels 0-1 are immune"
        assert sum(p["counts"]) == n_units(c["B"], c["h"], c["w"])
    nw = torch.cat([p["nwin"].reshape(-1) for _, p in out])
    ok = torch.cat([p["immune"].reshape(-1) for _, p in out])
    assert bool(((nw == ref.LF_CAP) & ok).any()), "no immune unit sits on the cap"
    assert bool(((nw > ref.LF_CAP) & (nw <= ref.LF_CAP + 32) & ok).any()), "no immune unit sits just above the cap"
    # (2, 2): an interior level-0 own-view tile stages exactly 12 rows x 16 columns = LF_CAP and must be tiled;
    # (2, 3): the same tile is 13 x 16 = 208, one row over
    B, h, w = STRETCH_MAP
    tx = (w + ref.LF_TX - 1) // ref.LF_TX
    t = 3 * tx + 3                                                                # pixels (6..7, 12..15)
    assert int(out[1][1]["nwin"][t, 0, 0]) == 12 * 16 == ref.LF_CAP
    assert int(out[2][1]["nwin"][t, 0, 0]) == 13 * 16
    return out


# ------------------------------------------------------------------------------------------------------------------------
# one launch, one case
# ------------------------------------------------------------------------------------------------------------------------
def launch(lib, c, dev, counts=False):
    B, h, w = c["B"], c["h"], c["w"]
    R = B * h * w

    def levels(f2):
        r = ref.rows(f2).to(dev)
        lv = [torch.empty(B * (h >> i) * (w >> i), c["C"], device=dev) for i in (1, 2, 3)]
        lib.feature_pyramid(r, lv, B, h, w)
        return [r] + lv
    outs = []
    for _ in range(2):
        t = torch.full((R, LD), float("nan"), device=dev)
        t[:, CORR_CH:] = SENT_F32
        outs.append(t)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev) if counts else None
    lib.dccl_lookup_feat(c["coords"].to(dev), ref.rows(c["f1a"]).to(dev), levels(c["f2a"]), ref.rows(c["f1b"]).to(dev),
                         levels(c["f2b"]), c["g"].to(dev), outs[0], outs[1], cnt)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return outs[0].cpu(), outs[1].cpu(), (None if cnt is None else [int(v) for v in cnt.cpu()])


def run_case(lib, c, dev, table, counts=False, repeats=True):
    """-> (failures, path counts or None).  The table row is (C family, map)."""
    fails = []
    name = f"{c['map']} {c['family']} C={c['C']}"
    own, raw, cnt = launch(lib, c, dev, counts)
    refs = reference(c)
    for what, got in (("own", own), ("raw", raw)):
        r = el.ratio(got[:, :CORR_CH], *refs[what])
        table.add(f"C={c['C']} {c['family']}", c["map"], r)
        if not r <= 1.0:
            fails.append(f"{name} {what}: |err|/bound = {r:.3g}")
        if not bool((got[:, CORR_CH:] == SENT_F32).all()):
            fails.append(f"{name} {what}: a padding column was written")
    if c["family"] == "outside":
        if not (bool((refs["own"][0] == 0).all()) and bool((own[:, :CORR_CH] == 0).all())):
            fails.append(f"{name}: the own view of a launch with no weighted corner is not exactly 0.0")
        if not float(refs["raw"][0].abs().max()) > 0.1:
            fails.append(f"{name}: the cross view has nothing to check")
    if cnt is not None and sum(cnt) != n_units(c["B"], c["h"], c["w"]):
        fails.append(f"{name}: path counts {cnt} do not add up to {n_units(c['B'], c['h'], c['w'])} units")
    if repeats:
        own2, raw2, _ = launch(lib, c, dev)
        if not (torch.equal(own2, own) and torch.equal(raw2, raw)):      # (NaN != NaN: an unwritten value fails here as well)
            fails.append(f"{name}: a second launch differs")
        N = c["h"] * c["w"]
        for b in range(c["B"] if c["B"] > 1 else 0):
            own1, raw1, _ = launch(lib, image_of(c, b), dev)
            if not (torch.equal(own1, own[b * N:(b + 1) * N]) and torch.equal(raw1, raw[b * N:(b + 1) * N])):
                fails.append(f"{name}: image {b} of the B = {c['B']} launch differs from its B = 1 launch")
    return fails, cnt
