"""References of the per-joint camera masks (include/jarvis_hip.h): the effective-set rule in numpy and the joint-masked
gather in fp32 torch on the CPU, on the gather indices of the pinned existing path (ReprojectionLayer.gather_indices)."""
import numpy as np
import torch


def effective_sets(jm, mask=None):
    """jm (T,J,C), mask (T,C) or None, anything numpy converts; nonzero = on -> e (T,J,C) uint8, n (T,J) int32:
    e = a && jm; a joint whose set is empty has the cameras of the camera mask (all of them without one)."""
    jm = np.asarray(jm) != 0
    T, J, C = jm.shape
    a = np.ones((T, C), bool) if mask is None else np.asarray(mask).reshape(T, C) != 0
    e = jm & a[:, None, :]
    empty = ~e.any(-1)
    e = np.where(empty[..., None], np.broadcast_to(a[:, None, :], e.shape), e)
    return e.astype(np.uint8), e.sum(-1).astype(np.int32)


def gather_ref(hm_pad, idx, e):
    """hm_pad (C,J,hs,hs) fp32 padded heat maps, idx (C,G,G,G) int64 gather indices, e (J,C) the effective sets ->
    vol (J,G,G,G) fp32: the camera-order fp32 sum, from +0, of the tapped values selected through torch.where(e, ., 0),
    divided in fp32 by the joint's number of cameras (1 for none)."""
    hm_pad, idx = hm_pad.cpu(), idx.cpu()
    e = torch.as_tensor(np.asarray(e) != 0)
    C, J = hm_pad.shape[:2]
    G = idx.shape[-1]
    vol = torch.zeros((J, G * G * G), dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    for c in range(C):
        taps = hm_pad[c].reshape(J, -1)[:, idx[c].reshape(-1)]                     # (J, G^3)
        vol = vol + torch.where(e[:, c, None], taps, zero)
    n = e.sum(1).clamp(min=1).to(torch.float32)
    return (vol / n[:, None]).reshape(J, G, G, G)
