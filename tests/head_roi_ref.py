"""The keypoint head's box in numpy: the rule csrc/reproject.hip's repro_box_kernel applies, the coarse
(u, v) field it applies it to, the window / tile arithmetic of csrc/deconv4.hip's box-relative tiling, and the small
geometries tests/test_hip_head_roi.py and tests/test_head_roi_cpu.py share.  A mirror for the tests, not an oracle of
the reference (which has no such box): the field is evaluated in float64, so against the fp32 kernel a box edge may sit
one pixel off where u / 2 or v / 2 is within rounding of an integer.
"""
import numpy as np

TILE_Y, TILE_X, EDGE_WINDOWS = 8, 16, 128      # csrc/deconv4.hip: kDTY, kDTX, windows per edge workgroup


def coarse_field(cam, intr, dist, center3d, center_hm, G, spacing, hs):
    """repro_coarse_kernel for one frame set: cam (C,4,3), intr (C,3,3), dist (C,1,5) or (C,5), center3d (3,) int,
    center_hm (C,2) int -> (C, Gh^3, 2) float64 (u, v) in padded-heat-map coordinates x 2, clamped to the crop."""
    cam, intr = np.asarray(cam, np.float64), np.asarray(intr, np.float64)
    dist = np.asarray(dist, np.float64).reshape(len(cam), -1)
    Gh = G // 2
    ax = (np.arange(Gh) - Gh // 2) * float(spacing) * 2.0
    gi, gj, gk = np.meshgrid(ax, ax, ax, indexing="ij")
    pts = np.stack([gi.ravel() + center3d[0], gj.ravel() + center3d[1], gk.ravel() + center3d[2],
                    np.ones(Gh ** 3)], 1)
    out = np.zeros((len(cam), Gh ** 3, 2))
    for c in range(len(cam)):
        q = pts @ cam[c]
        cx, cy, fx, fy = intr[c, 2, 0], intr[c, 2, 1], intr[c, 0, 0], intr[c, 1, 1]
        u, v = q[:, 0] / q[:, 2] - cx, q[:, 1] / q[:, 2] - cy
        r2 = (u / fx) ** 2 + (v / fy) ** 2
        d = 1.0 + (dist[c, 0] + dist[c, 1] * r2) * r2
        u, v = u * d + cx, v * d + cy
        chx, chy = float(center_hm[c][0]), float(center_hm[c][1])
        u = np.clip(u, chx - (hs - 1), chx + hs - 2) - chx + hs - 1
        v = np.clip(v, chy - (hs - 1), chy + hs - 2) - chy + hs - 1
        out[c, :, 0], out[c, :, 1] = u, v
    return out


def box_rule(umin, umax, vmin, vmax, Hh, heat_pad):
    """Stored-pixel box (x0, y0, x1, y1), inclusive, of a camera whose coarse field spans [umin, umax] x [vmin, vmax]:
    [trunc(min / 2) - 1 + heat_pad - 1, trunc(max / 2) - 1 + heat_pad + 1], clipped to the map."""
    sh = -1 + heat_pad
    lo = lambda m: min(max(int(m / 2.0) + sh - 1, 0), Hh - 1)
    hi = lambda m: max(min(int(m / 2.0) + sh + 1, Hh - 1), 0)
    return (lo(umin), lo(vmin), hi(umax), hi(vmax))


def boxes(field, Hh, heat_pad, valid=True, mask=None):
    """(C, Gh^3, 2) field -> (C, 4) boxes; a frame set that is not valid and a masked camera get the full map."""
    out = []
    for c in range(len(field)):
        if not valid or (mask is not None and not mask[c]):
            out.append((0, 0, Hh - 1, Hh - 1))
        else:
            out.append(box_rule(field[c, :, 0].min(), field[c, :, 0].max(), field[c, :, 1].min(), field[c, :, 1].max(),
                                Hh, heat_pad))
    return np.asarray(out, np.int32)


def windows(box):
    """Output pixel p belongs to window (p + 1) // 2: the box's first and last window per axis (x lo, y lo, x hi, y hi)."""
    return tuple((int(b) + 1) // 2 for b in box)


def pixel_box(wx_lo, wy_lo, wx_hi, wy_hi, H, W):
    """The windows [wx_lo, wx_hi] x [wy_lo, wy_hi] of an H x W input as an output-pixel box (window w holds the output
    pixels 2w - 1 and 2w; -1 and 2H / 2W do not exist)."""
    return (max(2 * wx_lo - 1, 0), max(2 * wy_lo - 1, 0), min(2 * wx_hi, 2 * W - 1), min(2 * wy_hi, 2 * H - 1))


def workgroups(box, H, W):
    """(interior tiles, edge workgroups) that compute something for an image with this box: the tiles laid from the
    box's first window up to its last interior one, the edge workgroups if the box reaches output row 2H - 1 or column
    2W - 1; without a box it is (ceil(H / 8) * ceil(W / 16), ceil((H + W + 1) / 128))."""
    wx_lo, wy_lo, wx_hi, wy_hi = windows(box)
    ny = -(-(min(wy_hi, H - 1) - wy_lo + 1) // TILE_Y)
    nx = -(-(min(wx_hi, W - 1) - wx_lo + 1) // TILE_X)
    edge = -(-(H + W + 1) // EDGE_WINDOWS) if (wy_hi >= H or wx_hi >= W) else 0
    return max(ny, 0) * max(nx, 0), edge


def all_workgroups(H, W):
    return -(-H // TILE_Y) * -(-W // TILE_X), -(-(H + W + 1) // EDGE_WINDOWS)


# ---- geometries of the box-against-gather test: G = 16, 3 - 4 cameras on the ring of synthetic.ring_calibration.
# tag -> (C, W, H, focal, bbox, G, spacing, frames [(centre mm, focal scale of that frame's calibration)])
#   plain : the cube well inside every crop
#   clamp : a short image and a long focal length: the crops are clamped at the image border, so the cube projects
#           partly outside them (the clamp branch of the coarse kernel)
#   frames: two frame sets with a calibration each (the second one's focal length 0.8 x) and centres of their own
GEOMETRIES = {
    "plain": (4, 640, 512, 900.0, 128, 16, 4, [((30.0, -20.0, 10.0), 1.0)]),
    "clamp": (3, 320, 256, 2400.0, 128, 16, 2, [((70.0, 60.0, -50.0), 1.0)]),
    "frames": (4, 640, 512, 900.0, 128, 16, 4, [((30.0, -20.0, 10.0), 1.0), ((-60.0, 45.0, -25.0), 0.8)]),
}


def geometry(tag):
    """-> dict of numpy / torch inputs: cam (T,C,4,3), intr (T,C,3,3), dist (T,C,5), center3d (T,3) int32, center_hm
    (T,C,2) int32 (clamped like jarvis3D.py:161-166), and the scalars."""
    import torch
    from jarvis_hybridnet_amd import synthetic as S
    C, W, H, focal, bbox, G, spacing, frames = GEOMETRIES[tag]
    cams, intrs, dists, c3, chm = [], [], [], [], []
    hw = bbox // 2
    for centre, fscale in frames:
        cam, intr, dist = S.ring_calibration(C, W, H, focal * fscale)
        uv = torch.from_numpy(S.project(np.asarray([centre]), cam, intr, dist))[:, 0]
        ch = uv.int()
        ch[:, 0] = ch[:, 0].clamp(min(hw, W - hw), max(hw, W - hw))
        ch[:, 1] = ch[:, 1].clamp(min(hw, H - hw), max(hw, H - hw))
        cams.append(cam); intrs.append(intr); dists.append(dist.reshape(C, 5))
        c3.append(torch.tensor(centre).int()); chm.append(ch)
    return dict(C=C, T=len(frames), G=G, spacing=spacing, hs=bbox // 2 + 2, Hh=bbox // 2,
                cam=torch.stack(cams).contiguous(), intr=torch.stack(intrs).contiguous(),
                dist=torch.stack(dists).contiguous(), center3d=torch.stack(c3).contiguous(),
                center_hm=torch.stack(chm).int().contiguous())


def geometry_boxes(g, heat_pad=0):
    """The mirror's boxes (T, C, 4) and fields of a geometry()."""
    fields = [coarse_field(g["cam"][t].numpy(), g["intr"][t].numpy(), g["dist"][t].numpy(), g["center3d"][t].numpy(),
                           g["center_hm"][t].numpy(), g["G"], g["spacing"], g["hs"]) for t in range(g["T"])]
    Hh = g["hs"] - 2 + 2 * heat_pad
    return np.stack([boxes(f, Hh, heat_pad) for f in fields]), fields
