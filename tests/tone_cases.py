"""The tone tables the GPU tests run under (tests/test_hip_tone.py) and the fp32 frames they define, shared with the CPU
test that checks the tables are usable (tests/test_tone_cpu.py): per-camera black level, white level, white-balance
gains and gamma near the identity, different for each of cfg2's four cameras so that a per-camera indexing mistake
changes the result."""
import numpy as np

from jarvis_hybridnet_amd import ToneTables

CAMERAS = 4
BLACK = (0.0, 4.0, 2.0, 6.0)
WHITE = (255.0, 250.0, 252.0, 246.0)
GAIN = ((1.00, 1.00, 1.00), (1.06, 1.00, 0.94), (0.95, 1.00, 1.08), (1.03, 0.98, 1.00))       # (R, G, B) per camera
GAMMA = (1.0, 1.1, 0.92, 1.05)


def tables():
    return ToneTables.from_curve(CAMERAS, black=BLACK, white=WHITE, gain=GAIN, gamma=GAMMA)


def other_tables():
    """A second set (the values a predictor is given under an existing recording): the cameras' curves rotated."""
    r = lambda v: tuple(v[1:]) + tuple(v[:1])  # noqa: E731
    return ToneTables.from_curve(CAMERAS, black=r(BLACK), white=r(WHITE), gain=r(GAIN), gamma=r(GAMMA))


def mapped_rgb(bgr, tone, cam0=0):
    """uint8 BGR (..., C, H, W, 3) -> fp32 RGB (..., C, 3, H, W): F[c][ch] = tables[cam0 + c][ch][bytes of channel ch],
    the frames the definition of the feature names (include/jarvis_hip.h)."""
    bgr = np.asarray(bgr)
    C = bgr.shape[-4]
    out = np.empty(bgr.shape[:-4] + (C, 3) + bgr.shape[-3:-1], dtype=np.float32)
    for c in range(C):
        for ch in range(3):
            out[..., c, ch, :, :] = tone.tables[cam0 + c, ch][bgr[..., c, :, :, 2 - ch]]
    return out
