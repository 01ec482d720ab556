"""Deterministic synthetic inputs for parity tests and the benchmark.

There is no network on the build or GPU machines, so every measurement and
parity case uses seeded random-init weights of the reference architecture,
a seeded ring calibration and Gaussian-blob frames.
Nothing here is arithmetic of the hot path itself.
"""
import math

import numpy as np
import torch

from . import arch

MEAN = [0.485, 0.456, 0.406]
STD = [0.229, 0.224, 0.225]


def _fill(spec, seed, deconv_std=1.2):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in spec:
        leaf = key.split(".")[-1]
        short = key.rsplit(".", 1)[0].split(".")[-1]
        if len(shape) == 1 and leaf != "bias":
            t = torch.rand(shape, generator=g) + 0.5           # fusion weights
        elif leaf == "bias":
            t = torch.randn(shape, generator=g) * 0.1
        elif short == "deconv1":
            t = torch.randn(shape, generator=g) * deconv_std
        elif short == "output_layer":
            t = torch.randn(shape, generator=g)
        elif short == "block" and "decoder_upsample1" in key:
            fan = shape[0]                                      # ConvT: in-channels
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan)
        else:
            fan = int(np.prod(shape[1:]))
            t = torch.randn(shape, generator=g) * math.sqrt(2.0 / fan)
        sd[key] = t.float().contiguous()
    return sd


def efficienttrack_weights(model_size, num_joints, seed, deconv_std=1.2):
    return _fill(arch.efficienttrack_params(model_size, num_joints), seed, deconv_std)


def v2v_weights(num_joints, seed):
    return _fill(arch.v2v_params(num_joints), seed)


def hybridnet_weights(model_size, num_joints, seed, deconv_std=1.2):
    return _fill(arch.hybridnet_params(model_size, num_joints), seed, deconv_std)


def ring_cameras(num_cameras, width, height, focal=1800.0, radius=1500.0, k1=-0.05, k2=0.01):
    """Per-camera (R (3,3), T (3,), Kt (3,3), dist (5,)) in the convention of the
    reference's calibration files (row-vector: x_cam = X @ R + T, pixel_h = x_cam @ Kt)."""
    cams = []
    for i in range(num_cameras):
        th = 2.0 * math.pi * i / num_cameras
        ph = 0.3 * math.sin(3.0 * th)
        pos = radius * np.array([math.cos(th) * math.cos(ph),
                                 math.sin(th) * math.cos(ph), math.sin(ph)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        rwc = np.stack([x, y, z], 0)
        kt = np.array([[focal, 0, 0], [0, focal, 0], [width / 2.0, height / 2.0, 1.0]])
        cams.append((rwc.T, -pos @ rwc.T, kt, np.array([k1, k2, 0.0, 0.0, 0.0])))
    return cams


def write_opencv_yaml(path, R, T, Kt, dist):
    """One camera in the OpenCV FileStorage YAML layout the reference reads
    (datasets/*/calib_params/*/*.yaml: intrinsicMatrix, distortionCoefficients, R, T)."""
    def mat(name, a, rows, cols):
        data = ", ".join(repr(float(v)) for v in np.asarray(a, dtype=np.float64).reshape(-1))
        return "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s ]\n" % (
            name, rows, cols, data)
    with open(path, "w") as f:
        f.write("%YAML:1.0\n---\n")
        f.write(mat("intrinsicMatrix", Kt, 3, 3))
        f.write(mat("distortionCoefficients", dist, 1, 5))
        f.write(mat("R", R, 3, 3))
        f.write(mat("T", T, 3, 1))


def ring_calibration(num_cameras, width, height, focal=1800.0, radius=1500.0,
                     k1=-0.05, k2=0.01):
    """Cameras on a ring looking at the origin, in the reference's storage
    convention (utils/reprojection.py:33-39,105-107): cameraMatrices (C,4,3) =
    [R;T] @ Kt, intrinsicMatrices (C,3,3) = Kt with the principal point in row
    2, distortionCoefficients (C,1,5) with k1,k2 in the first two slots."""
    cam = np.zeros((num_cameras, 4, 3))
    intr = np.zeros((num_cameras, 3, 3))
    dist = np.zeros((num_cameras, 1, 5))
    for i in range(num_cameras):
        th = 2.0 * math.pi * i / num_cameras
        ph = 0.3 * math.sin(3.0 * th)
        pos = radius * np.array([math.cos(th) * math.cos(ph),
                                 math.sin(th) * math.cos(ph), math.sin(ph)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(z, np.array([0.0, 0.0, 1.0]))
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        rwc = np.stack([x, y, z], 0)            # rows = camera axes in world
        R = rwc.T
        T = -pos @ rwc.T
        kt = np.array([[focal, 0, 0], [0, focal, 0], [width / 2.0, height / 2.0, 1.0]])
        cam[i] = np.concatenate([R, T[None]], 0) @ kt
        intr[i] = kt
        dist[i, 0, 0], dist[i, 0, 1] = k1, k2
    return (torch.from_numpy(cam).float(), torch.from_numpy(intr).float(),
            torch.from_numpy(dist).float())


def project(points, cam, intr, dist):
    """float64 pinhole + 2-term radial projection of (P,3) points -> (C,P,2)."""
    cam, intr, dist = (t.double().numpy() for t in (cam, intr, dist))
    ph = np.concatenate([points, np.ones((points.shape[0], 1))], 1)
    out = np.zeros((cam.shape[0], points.shape[0], 2))
    for c in range(cam.shape[0]):
        q = ph @ cam[c]
        u = q[:, 0] / q[:, 2] - intr[c, 2, 0]
        v = q[:, 1] / q[:, 2] - intr[c, 2, 1]
        r2 = (u / intr[c, 0, 0]) ** 2 + (v / intr[c, 1, 1]) ** 2
        d = 1 + (dist[c, 0, 0] + dist[c, 0, 1] * r2) * r2
        out[c, :, 0] = u * d + intr[c, 2, 0]
        out[c, :, 1] = v * d + intr[c, 2, 1]
    return out


def blob_frames(calib, width, height, num_joints, seed, sigma=6.0, amp=0.9):
    """(C,3,H,W) fp32 RGB frames in [0,1]: dim noise plus one Gaussian blob per
    joint at the projection of a random 3D skeleton.  Returns (frames,
    joints3d (J,3), centre (3,))."""
    cam, intr, dist = calib
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-100, 100, 3)
    joints = centre + rng.uniform(-40, 40, (num_joints, 3))
    uv = project(joints, cam, intr, dist)
    C = cam.shape[0]
    g = torch.Generator().manual_seed(seed)
    frames = torch.rand((C, 3, height, width), generator=g) * 0.05
    r = int(4 * sigma)
    ax = torch.arange(-r, r + 1, dtype=torch.float32)
    for c in range(C):
        for j in range(num_joints):
            u, v = uv[c, j]
            iu, iv = int(round(u)), int(round(v))
            if iu - r < 0 or iv - r < 0 or iu + r >= width or iv + r >= height:
                continue
            gx = torch.exp(-((ax + iu - float(u)) ** 2) / (2 * sigma * sigma))
            gy = torch.exp(-((ax + iv - float(v)) ** 2) / (2 * sigma * sigma))
            blob = amp * gy[:, None] * gx[None, :]
            col = 0.5 + 0.5 * torch.tensor([math.sin(j), math.cos(2 * j), math.sin(3 * j + 1)])
            frames[c, :, iv - r:iv + r + 1, iu - r:iu + r + 1] += col.view(3, 1, 1) * blob
    return frames.clamp_(0, 1), joints, centre


def smooth_heatmaps(num_cameras, num_joints, size, seed):
    """Smooth positive (C,J,size,size) heatmap field in 0..255 units used by
    stage-level reprojection tests."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32),
                            torch.arange(size, dtype=torch.float32), indexing="ij")
    out = torch.zeros(num_cameras, num_joints, size, size)
    for c in range(num_cameras):
        for j in range(num_joints):
            cx, cy = (torch.rand(2, generator=g) * size).tolist()
            s = 4.0 + 10.0 * torch.rand(1, generator=g).item()
            a = 60.0 + 190.0 * torch.rand(1, generator=g).item()
            out[c, j] = a * torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return out + torch.rand(out.shape, generator=g) * 2.0


def pack_yuv420(y, u, v, fmt):
    """Planes Y (..., H, W), U and V (..., H/2, W/2) uint8 -> (..., 3H/2, W) uint8 in the layout `fmt`:
    'i420' = Y, then U, then V; 'nv12' = Y, then one interleaved plane, U first."""
    y, u, v = np.asarray(y, np.uint8), np.asarray(u, np.uint8), np.asarray(v, np.uint8)
    lead, (H, W) = y.shape[:-2], y.shape[-2:]
    if fmt == "i420":
        chroma = np.concatenate([u.reshape(lead + (-1,)), v.reshape(lead + (-1,))], -1).reshape(lead + (H // 2, W))
    elif fmt == "nv12":
        chroma = np.stack([u, v], -1).reshape(lead + (H // 2, W))
    else:
        raise ValueError("fmt must be 'i420' or 'nv12', got %r" % (fmt,))
    return np.ascontiguousarray(np.concatenate([y, chroma], -2))


def bgr_to_yuv420(bgr, fmt):
    """uint8 BGR (..., H, W, 3), H and W even -> YUV 4:2:0 (..., 3H/2, W) in the layout `fmt`: a forward BT.601
    limited-range transform with 2 x 2 averaged chroma (test data; only the inverse, the conversion the kernels
    apply, is a contract)."""
    x = np.asarray(bgr, np.float32)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    y = 16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b
    u = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    v = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b

    def pool(p):
        return 0.25 * (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2])

    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)  # noqa: E731
    return pack_yuv420(q(y), q(pool(u)), q(pool(v)), fmt)


def reduce_samples(a, shift):
    """Samples wider than a byte -> the bytes the fetch makes of them: min(sample >> shift, 255), uint8 (the
    truncation a camera applies when its PixelFormat goes from Mono12 to Mono8; a sample with bits above the declared
    depth saturates)."""
    a = np.asarray(a)
    if a.dtype.kind not in "ui":
        raise ValueError("reduce_samples takes integer samples, got %s" % a.dtype)
    return np.minimum(a.astype(np.uint32) >> shift, 255).astype(np.uint8)


def widen(bytes_, shift, rng, saturate=False):
    """uint8 bytes -> uint16 samples with random low `shift` bits that reduce_samples(., shift) takes back to the
    bytes.  saturate (the second variant, shift < 8): where a byte is 255, about half of the samples also get random
    bits ABOVE the declared depth of 8 + shift bits -- they still reduce to 255, by saturation."""
    b = np.asarray(bytes_, np.uint8)
    if not 0 <= shift <= 8:
        raise ValueError("shift must be 0..8, got %r" % (shift,))
    out = (b.astype(np.uint16) << shift) | rng.integers(0, 1 << shift, b.shape, dtype=np.uint16)
    if saturate and shift < 8:
        over = rng.integers(0, 1 << (8 - shift), b.shape, dtype=np.uint16) << (8 + shift)
        out = np.where((b == 255) & (rng.integers(0, 2, b.shape) == 1), out | over, out).astype(np.uint16)
    return out


def pack_bits(samples, bits):
    """Rows of samples (..., W) -> the GenICam PFNC 10p / 12p bytes (..., ceil(bits * W / 8)) uint8: every row a
    little-endian bit stream, sample x at bits [bits * x, bits * x + bits); the unused high bits of a row's last
    byte are 0.  Samples are taken modulo 2^bits."""
    a = np.asarray(samples).astype(np.uint16)
    W = a.shape[-1]
    stream = ((a[..., None] >> np.arange(bits, dtype=np.uint16)) & 1).astype(np.uint8).reshape(a.shape[:-1] + (W * bits,))
    return np.packbits(stream, axis=-1, bitorder="little")


def unpack_bits(packed, bits, width):
    """The inverse of pack_bits: (..., ceil(bits * width / 8)) uint8 -> (..., width) uint16 (test of the packer)."""
    stream = np.unpackbits(np.asarray(packed, np.uint8), axis=-1, bitorder="little")[..., :bits * width]
    stream = stream.reshape(stream.shape[:-1] + (width, bits)).astype(np.uint16)
    return (stream << np.arange(bits, dtype=np.uint16)).sum(-1, dtype=np.uint16)


def _le16(a):
    """uint16 (..., W) -> their little-endian bytes (..., 2W) uint8."""
    a = np.asarray(a).astype("<u2")
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[:-1] + (2 * a.shape[-1],))


def pack_yuv_surface(y, u, v, surface, fill=0):
    """Planes Y (..., H, W), U and V (..., H/2, W/2) uint8 -> (..., image_stride) uint8 laid out as the YuvSurface
    `surface` describes; every byte that belongs to no plane (pitch padding, the rows between the planes, the gap up
    to image_stride) is `fill`.  A 16-bit description (surface.bits > 8) takes uint16 planes and writes every sample
    as two little-endian bytes."""
    if surface.sample:
        return _pack_yuv_surface16(y, u, v, surface, fill)
    y, u, v = np.asarray(y, np.uint8), np.asarray(u, np.uint8), np.asarray(v, np.uint8)
    s, lead = surface, y.shape[:-2]
    H, W = s.height, s.width
    if y.shape[-2:] != (H, W) or u.shape != lead + (H // 2, W // 2) or v.shape != u.shape:
        raise ValueError("planes %s / %s / %s do not fit a %d x %d surface" % (y.shape, u.shape, v.shape, H, W))
    out = np.full(lead + (s.image_stride,), fill, np.uint8)

    def put(plane, offset, pitch, step):
        rows, cols = plane.shape[-2:]
        idx = offset + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :] * step
        out[..., idx.reshape(-1)] = plane.reshape(lead + (-1,))

    put(y, s.y_offset, s.y_pitch, 1)
    put(u, s.u_offset, s.c_pitch, s.c_step)
    put(v, s.v_offset, s.c_pitch, s.c_step)
    return out


def _pack_yuv_surface16(y, u, v, surface, fill):
    y, u, v = (np.asarray(p) for p in (y, u, v))
    if any(p.dtype != np.uint16 for p in (y, u, v)):
        raise ValueError("a 16-bit surface takes uint16 planes, got %s / %s / %s" % (y.dtype, u.dtype, v.dtype))
    s, lead = surface, y.shape[:-2]
    H, W = s.height, s.width
    if y.shape[-2:] != (H, W) or u.shape != lead + (H // 2, W // 2) or v.shape != u.shape:
        raise ValueError("planes %s / %s / %s do not fit a %d x %d surface" % (y.shape, u.shape, v.shape, H, W))
    out = np.full(lead + (s.image_stride,), fill, np.uint8)

    def put(plane, offset, pitch, step):
        rows, cols = plane.shape[-2:]
        idx = offset + np.arange(rows)[:, None, None] * pitch + np.arange(cols)[None, :, None] * (2 * step) \
            + np.arange(2)[None, None, :]
        out[..., idx.reshape(-1)] = _le16(plane).reshape(lead + (-1,))

    put(y, s.y_offset, s.y_pitch, 1)
    put(u, s.u_offset, s.c_pitch, s.c_step)
    put(v, s.v_offset, s.c_pitch, s.c_step)
    return out


def bgr_to_yuv(bgr, matrix="bt601", range="limited"):
    """uint8 BGR (..., H, W, 3), H and W even -> planes (Y (..., H, W), U, V (..., H/2, W/2)) uint8: the forward
    transform of `matrix` ('bt601' | 'bt709') and `range` ('limited' | 'full') in float64, rounded and clamped, with
    2 x 2 chroma means (test data: a frame decoded with the matching matrix looks like the original; only the
    inverse is a contract)."""
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    sy, sc, y0 = {"limited": (219.0 / 255.0, 224.0 / 255.0, 16.0), "full": (1.0, 1.0, 0.0)}[range]
    x = np.asarray(bgr, np.float64)
    b, g, r = x[..., 0], x[..., 1], x[..., 2]
    luma = kr * r + (1.0 - kr - kb) * g + kb * b
    y = y0 + sy * luma
    u = 128.0 + sc * (b - luma) / (2.0 * (1.0 - kb))
    v = 128.0 + sc * (r - luma) / (2.0 * (1.0 - kr))

    def pool(p):
        return 0.25 * (p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2])

    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)  # noqa: E731
    return q(y), q(pool(u)), q(pool(v))


# red site (row parity, column parity) of a Bayer pattern's top-left 2 x 2 cell; blue sits diagonally opposite
_BAYER_RED = {"rggb": (0, 0), "bggr": (1, 1), "grbg": (0, 1), "gbrg": (1, 0)}


def mosaic(bgr, pattern):
    """uint8 BGR (..., H, W, 3) -> the raw (..., H, W) uint8 image a sensor with the colour filter `pattern` stores:
    'mono' keeps the green channel, a Bayer pattern ('rggb' | 'bggr' | 'grbg' | 'gbrg') the one sample of each
    pixel's site (test data: the inverse, sensor_to_bgr, is the contract)."""
    x = np.asarray(bgr, np.uint8)
    if pattern == "mono":
        return np.ascontiguousarray(x[..., 1])
    ry, rx = _BAYER_RED[pattern]
    raw = np.ascontiguousarray(x[..., 1])                        # green everywhere, then the red and blue sites
    raw[..., ry::2, rx::2] = x[..., ry::2, rx::2, 2]
    raw[..., 1 - ry::2, 1 - rx::2] = x[..., 1 - ry::2, 1 - rx::2, 0]
    return raw


def sensor_to_bgr(raw, pattern):
    """The numpy reference of the sensor conversion (include/jarvis_hip.h), in int32: raw (..., H, W) uint8 ->
    (..., H, W, 3) uint8 BGR.  'mono': the byte three times.  Bayer: every pixel is first clamped to the interior
    (1..H-2, 1..W-2) and the clamped pixel demosaiced -- at a red or blue site green = (N+S+E+W+2) >> 2 and the
    opposite colour = (NW+NE+SW+SE+2) >> 2, at a green site the left/right colour = (W+E+1) >> 1 and the above/below
    colour = (N+S+1) >> 1."""
    raw = np.asarray(raw, np.uint8)
    if pattern == "mono":
        return np.repeat(raw[..., None], 3, axis=-1)
    ry, rx = _BAYER_RED[pattern]
    H, W = raw.shape[-2:]
    if H < 4 or W < 4 or H % 2 or W % 2:
        raise ValueError("Bayer frames need an even height and width of at least 4; got %d x %d" % (H, W))
    r32 = raw.astype(np.int32)
    y = np.clip(np.arange(H), 1, H - 2)[:, None]
    x = np.clip(np.arange(W), 1, W - 2)[None, :]

    def at(dy, dx):
        return r32[..., y + dy, x + dx]

    own = at(0, 0)
    cross = (at(-1, 0) + at(1, 0) + at(0, 1) + at(0, -1) + 2) >> 2
    diag = (at(-1, -1) + at(-1, 1) + at(1, -1) + at(1, 1) + 2) >> 2
    lr = (at(0, -1) + at(0, 1) + 1) >> 1
    ab = (at(-1, 0) + at(1, 0) + 1) >> 1
    py, px = (y & 1) ^ ry, (x & 1) ^ rx                          # (0, 0): red site, (1, 1): blue site, else green
    red_site, blue_site = (py == 0) & (px == 0), (py == 1) & (px == 1)
    green_red_row = (py == 0) & (px == 1)                        # red left and right, blue above and below
    g = np.where(red_site | blue_site, cross, own)
    r = np.where(red_site, own, np.where(blue_site, diag, np.where(green_red_row, lr, ab)))
    b = np.where(blue_site, own, np.where(red_site, diag, np.where(green_red_row, ab, lr)))
    return np.stack([b, g, r], axis=-1).astype(np.uint8)


def pack_sensor_surface(raw, surface, fill=0):
    """raw (..., H, W) uint8 -> (..., image_stride) uint8 laid out as the SensorSurface `surface` describes; every
    byte that is no sample (the bytes before `offset`, pitch padding, the gap up to image_stride) is `fill`.
    A wide description (surface.container != 'u8') takes uint16 samples: the 16-bit containers store them as two
    little-endian bytes, 'packed' as the 10p / 12p bit stream of each row (pack_bits) -- there the unused high bits of
    a row's last byte take the bits of `fill` too."""
    s = surface
    wide = s.container != "u8"
    raw = np.asarray(raw) if wide else np.asarray(raw, np.uint8)
    if wide and raw.dtype != np.uint16:
        raise ValueError("a %r surface takes uint16 samples, got %s" % (s.container, raw.dtype))
    lead = raw.shape[:-2]
    if raw.shape[-2:] != (s.height, s.width):
        raise ValueError("raw %s does not fit a %d x %d surface" % (raw.shape, s.height, s.width))
    out = np.full(lead + (s.image_stride,), fill, np.uint8)
    rows = raw
    if s.container == "packed":
        rows = pack_bits(raw, s.bits)
        spare = 8 * rows.shape[-1] - s.bits * s.width           # unused high bits of the last byte of a row
        if spare:
            rows[..., -1] |= (fill & 0xff) >> (8 - spare) << (8 - spare)
    elif wide:
        rows = _le16(raw)
    nb = rows.shape[-1]
    idx = s.offset + np.arange(s.height)[:, None] * s.pitch + np.arange(nb)[None, :]
    out[..., idx.reshape(-1)] = rows.reshape(lead + (-1,))
    return out


def _component_index(s, k):
    """Byte offsets (H, W) of component k of every pixel of a PixelSurface image."""
    y = (np.arange(s.height) >> s.ys[k])[:, None]
    x = (np.arange(s.width) >> s.xs[k])[None, :]
    return s.offset[k] + y * s.pitch[k] + x * s.step[k]


def pixels_to_bgr(buf, surface):
    """The numpy reference of the pixel-surface fetch (include/jarvis_hip.h): buf (..., image_stride) uint8 laid out as
    the PixelSurface `surface` describes -> (..., H, W, 3) uint8 BGR.  Component k of pixel (y, x) is the byte at
    offset[k] + (y >> ys[k]) * pitch[k] + (x >> xs[k]) * step[k]; colour 'yuv' converts (Y, U, V) in int32 with the
    constants of the surface's matrix and range (the arithmetic of a YuvSurface), chroma replicated."""
    s = surface
    buf = np.asarray(buf, np.uint8)
    if buf.shape[-1] != s.image_stride:
        raise ValueError("buf %s does not hold images of %d bytes" % (buf.shape, s.image_stride))
    c = [buf[..., _component_index(s, k)].astype(np.int32) for k in range(3)]
    if s.colour == "yuv":
        y0, cy, cvr, cub, cug, cvg = s.coefficients
        u, v = c[1] - 128, c[2] - 128
        yy = np.maximum(c[0] - y0, 0) * cy + (1 << 19)
        c = [(yy + cvr * v) >> 20, (yy + cvg * v + cug * u) >> 20, (yy + cub * u) >> 20]
    return np.stack([np.clip(c[2], 0, 255), np.clip(c[1], 0, 255), np.clip(c[0], 0, 255)], axis=-1).astype(np.uint8)


def pack_pixel_surface(planes_or_bgr, surface, fill=0):
    """Test data laid out as the PixelSurface `surface` describes -> (..., image_stride) uint8; every byte that is no
    component (an alpha byte, pitch padding, gaps, the bytes before the first offset) is `fill`.  colour 'rgb': uint8
    BGR (..., H, W, 3).  colour 'yuv': the planes (Y (..., H, W), U, V (..., ceil(H / 2^ys), ceil(W / 2^xs)))."""
    s = surface
    H, W = s.height, s.width
    if s.colour == "rgb":
        bgr = np.asarray(planes_or_bgr, np.uint8)
        if bgr.shape[-3:] != (H, W, 3):
            raise ValueError("bgr %s does not fit a %d x %d surface" % (bgr.shape, H, W))
        planes = [bgr[..., 2], bgr[..., 1], bgr[..., 0]]
    else:
        planes = [np.asarray(p, np.uint8) for p in planes_or_bgr]
        want = [(((H - 1) >> s.ys[k]) + 1, ((W - 1) >> s.xs[k]) + 1) for k in range(3)]
        if len(planes) != 3 or any(p.shape[-2:] != w for p, w in zip(planes, want)):
            raise ValueError("planes %s do not fit a %d x %d surface (%s)" % ([p.shape for p in planes], H, W, want))
    lead = planes[0].shape[:-2]
    out = np.full(lead + (s.image_stride,), fill, np.uint8)
    for k, plane in enumerate(planes):
        rows, cols = plane.shape[-2:]
        idx = s.offset[k] + np.arange(rows)[:, None] * s.pitch[k] + np.arange(cols)[None, :] * s.step[k]
        out[..., idx.reshape(-1)] = plane.reshape(lead + (-1,))
    return out
