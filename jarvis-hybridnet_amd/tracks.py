"""Subject identity across frame sets: the tracker behind detect_subjects (jh_op_track_subjects, include/jarvis_hip.h).
Importing this module loads neither the library nor torch; making a SubjectTracker does."""
from typing import NamedTuple

from .subjects import Subjects


class Tracks(NamedTuple):
    """What a SubjectTracker says about the rows it returns, int32 device tensors: ids (T,K) the identity of the track in
    slot k after frame set t (-1: the slot is free) -- the one number that names an animal for the whole run --; slots
    (T,K) the row of the detect_subjects call the slot holds in frame set t, or -1; missed (T,K) the frame sets since the
    track's last match (0: matched or born in this frame set, -1: free); dropped (T,) the present detections of frame
    set t that found neither a track nor a free slot."""
    ids: object
    slots: object
    missed: object
    dropped: object


def check_tracker(tracker, max_subjects):
    """The `tracker` argument of the subject calls: None, or a SubjectTracker of max_subjects slots (ValueError)."""
    if tracker is None:
        return None
    if not isinstance(tracker, SubjectTracker):
        raise ValueError("tracker must be a SubjectTracker or None, got %s" % type(tracker).__name__)
    if tracker.max_subjects != max_subjects:
        raise ValueError("the tracker has %d slots; this call detects %r subjects" % (tracker.max_subjects, max_subjects))
    return tracker


class SubjectTracker:
    """Up to `max_subjects` tracks in device memory (a jh_track_state), matched against the subjects of every frame set
    by one small kernel: greedy, nearest first, gated at `max_jump_mm` per elapsed frame set; the definition, step by
    step, is the header's.  max_jump_mm has no default: it is the rig's.  max_missed (0), predict (True) and coast
    (False) are documented values, not recommendations (_native.track_params).

    update(subjects) -> (Subjects in slot order, Tracks): row (t, k) of the result is the row (t, slots[t, k]) of what
    came in, or an empty row (NaN centre, views 0, members -1, NaN error) -- with coast=True the predicted centre of a
    track that is alive and unmatched.  The frame sets of one update are consecutive in time, and so are successive
    updates.  It launches on the current stream and waits -- on the device, through an event -- for the tracker's
    previous update or reset on whatever stream that ran: updates take effect in call order, also when the batches of a
    recording go round the streams of a MultiStreamPredictor.  No host synchronisation.
    reset(): every slot free, next_id 0.  state(): a host copy for debugging (synchronises)."""

    def __init__(self, max_subjects, max_jump_mm, max_missed=0, predict=True, coast=False, device="cuda"):
        import torch
        from . import _native as N
        self.params = N.track_params(max_subjects, max_jump_mm, max_missed, predict, coast)
        self.max_subjects = int(max_subjects)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("jarvis_hybridnet_amd needs a CUDA (HIP) device; got %r" % (device,))
        self._state = torch.empty((N.ctypes.sizeof(N.TrackStateStruct),), dtype=torch.uint8, device=self.device)
        self._event = None
        self.reset()

    def _ordered(self):
        """The current stream, made to wait for the last launch on this tracker's state."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if self._event is not None:
            cur.wait_event(self._event)
        self._state.record_stream(cur)                      # (allocated on another stream, perhaps)
        return cur

    def _launched(self, cur):
        import torch
        self._event = torch.cuda.Event()
        self._event.record(cur)

    def reset(self):
        """All slots free, next_id 0 (jh_op_track_reset), on the current stream, ordered like an update."""
        from . import _native as N
        cur = self._ordered()
        N.check(N.lib().jh_op_track_reset(N.ptr(self._state), cur.cuda_stream))
        self._launched(cur)

    def update(self, subjects):
        """subjects: a Subjects (what detect_subjects returned), or any four (centers, views, members, error) with
        centers (T,K,3) float32 and views (T,K) / members (T,K,C) int32 / error (T,K) float32 -- the last three may be
        None together: centres alone --, contiguous device tensors, K = max_subjects.  -> (Subjects, Tracks)."""
        import ctypes
        import torch
        from . import _native as N
        centers, views, members, error = subjects
        K = self.max_subjects
        ok = (torch.is_tensor(centers) and centers.is_cuda and centers.dtype == torch.float32 and centers.dim() == 3
              and tuple(centers.shape[1:]) == (K, 3) and centers.shape[0] >= 1 and centers.is_contiguous())
        if not ok:
            raise ValueError("centers must be a contiguous (T, %d, 3) float32 device tensor with T >= 1; got %s"
                             % (K, tuple(centers.shape) if torch.is_tensor(centers) else type(centers).__name__))
        T, dev = int(centers.shape[0]), centers.device
        rest = (views, members, error)
        if any(t is None for t in rest) and not all(t is None for t in rest):
            raise ValueError("views, members and error are given together or not at all")
        cams = 1
        if views is not None:
            wanted = ((views, torch.int32, (T, K)), (members, torch.int32, (T, K, None)), (error, torch.float32, (T, K)))
            for name, (t, dtype, shape) in zip(("views", "members", "error"), wanted):
                fits = (torch.is_tensor(t) and t.device == dev and t.dtype == dtype and t.dim() == len(shape)
                        and all(w is None or int(g) == w for g, w in zip(t.shape, shape)) and t.is_contiguous())
                if not fits or t.numel() == 0:
                    raise ValueError("%s must be a contiguous %s device tensor of shape %s beside centers %s"
                                     % (name, dtype, tuple("C" if w is None else w for w in shape),
                                        tuple(centers.shape)))
            cams = int(members.shape[2])
        out = Subjects(torch.empty_like(centers), *(None if t is None else torch.empty_like(t) for t in rest))
        tracks = Tracks(*(torch.empty((T, K), device=dev, dtype=torch.int32) for _ in range(3)),
                        torch.empty((T,), device=dev, dtype=torch.int32))
        cur = self._ordered()
        N.check(N.lib().jh_op_track_subjects(*(N.ptr(t) for t in (centers,) + rest), T, cams, ctypes.byref(self.params),
                                             N.ptr(self._state), *(N.ptr(t) for t in out), *(N.ptr(t) for t in tracks),
                                             cur.cuda_stream))
        self._launched(cur)
        return out, tracks

    def state(self):
        """A host copy of the jh_track_state, for debugging: dict of numpy arrays pos (8,3), vel (8,3), missed (8,),
        id (8,) and the int next_id.  Waits for the last update (a host synchronisation)."""
        import numpy as np
        from . import _native as N
        self._ordered()
        raw = self._state.cpu().numpy().tobytes()
        s = N.TrackStateStruct.from_buffer_copy(raw)
        return dict(pos=np.array(s.pos, np.float32).reshape(8, 3), vel=np.array(s.vel, np.float32).reshape(8, 3),
                    missed=np.array(s.missed, np.int32), id=np.array(s.id, np.int32), next_id=int(s.next_id))
