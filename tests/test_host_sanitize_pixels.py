"""CPU: the pixel-surface host code under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.

tests/host_sanitize_pixels/Makefile compiles the host halves of csrc/api_frames.hip and csrc/preprocess.hip with
-fsanitize=address,undefined and links them with sweep.cpp (its own main) against the malloc-backed HIP stand-in of
tests/host_sanitize.  The program sweeps jh_pixel_surface_check, the FrameSource construction and the host path of
jh_op_pixels_to_bgr over 400 000 random and extreme descriptions (int64 / int32 limits in every field) and checks that
an accepted description addresses no byte outside the image.  Nothing is preloaded and no Python loads the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "host_sanitize_pixels")


def test_pixel_surface_host_code_under_asan_ubsan():
    build = subprocess.run(["make", "-C", SAN, "-j4"], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([os.path.join(SAN, "build", "sweep")], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=600)
    tail = run.stdout[-2000:] + run.stderr[-4000:]
    assert run.returncode == 0, tail
    assert run.stdout.startswith("sweep OK: "), tail
    for marker in ("AddressSanitizer", "runtime error:", "UndefinedBehaviorSanitizer"):
        assert marker not in run.stderr, tail
