"""The subjects a detect_subjects call returns (pure Python: no library, no torch)."""
from typing import NamedTuple


class Subjects(NamedTuple):
    """Up to K subjects per frame set, found by grouping the top local maxima of every camera's centre heat map across
    cameras (jh_predictor_detect_subjects, include/jarvis_hip.h): centers (T,K,3) world millimetres, NaN for an empty
    subject -- what `centers=` of forward_batch / forward_images takes, an empty subject being an invalid row --;
    views (T,K) int32 the number of cameras that support the subject (0 when empty); members (T,K,C) int32 the slot of
    the supporting peak of every camera or -1; error (T,K) the mean distance in full-frame pixels between the members'
    peaks and the projection of the centre (NaN when empty).  Subjects are ordered by (views descending, cost
    ascending) within ONE frame set: subject k of frame set t and of t+1 are unrelated, unless a tracks.SubjectTracker put
    them into slot order (detect_subjects(..., tracker=))."""
    centers: object
    views: object
    members: object
    error: object
