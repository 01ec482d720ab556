"""MI355X-native implementation of the JARVIS-HybridNet multi-view inference
hot path (EfficientTrack 2D CNN -> ReprojectionLayer -> V2V 3D CNN ->
soft-argmax) behind the reference's own Python API.

All arithmetic on the path runs in hand-written HIP kernels for gfx950 that
live in `csrc/` and are reached through the C ABI declared in
`include/jarvis_hip.h` (`libjarvis_hip.so`).  There is no CPU fallback: every
entry point raises if the library cannot be loaded.
"""
__version__ = "0.1.0"

from .yuv_surface import YuvSurface  # noqa: E402,F401 -- pure Python: importing the package still loads no library
from .sensor_surface import SensorSurface  # noqa: E402,F401 -- likewise
from .pixel_surface import PixelSurface  # noqa: E402,F401 -- likewise
from .tone import ToneTables  # noqa: E402,F401 -- likewise
from .spread import Spread3D # noqa: E402,F401 -- likewise
from .subjects import Subjects  # noqa: E402,F401 -- likewise
from .triangulated import Triangulated3D  # noqa: E402,F401 -- likewise
from .joint_mask import JointMask  # noqa: E402,F401 -- likewise
from .tracks import SubjectTracker, Tracks  # noqa: E402,F401 -- likewise (a SubjectTracker loads it when it is made)
