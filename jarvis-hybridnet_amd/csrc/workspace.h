// Workspaces carved out of one block: the Carver, and the one way a "first call allocates" workspace is made.
// Host only and free of HIP: the allocator and the capture check come in as arguments (predictor.h gives the
// predictor's own), so tests/workspace_smoke.cpp builds this header alone with a host compiler.
#pragma once
#include <cstddef>

namespace jh {

// A block carved into 256-byte aligned pieces, in the order they are taken.  With base == nullptr it only measures
// (jh_*_workspace_bytes): every piece is null and `off` ends at the bytes the block needs.  payload: the bytes asked
// for, without the padding.
struct Carver {
  char* base;
  size_t cap, off = 0, payload = 0;
  Carver(void* b, size_t c) : base(static_cast<char*>(b)), cap(c) {}
  template <typename T> T* take(size_t count) {
    const size_t at = off;
    off += (count * sizeof(T) + 255) / 256 * 256;
    payload += count * sizeof(T);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  bool fits() const { return off <= cap; }
};

struct CarveSizes { size_t bytes = 0, payload = 0; };   // the block as allocated; the sum of the pieces as asked for

// A workspace that the first call of its kind allocates.  lay(Carver&, Pieces&) describes the pieces ONCE, as
// c.take<T>(count) lines: it runs on a null base to measure and, after ONE allocation, on the block.
//   check_capture(what)   -> non-zero inside a stream capture, having reported `what`, the site's own message
//                            (what == nullptr: the site has no stream to ask and the check is not made);
//   alloc(void**, bytes)  -> non-zero on failure.
// *out (and *sizes) are written only when everything succeeded: on any failure nothing of the caller's is touched, so a
// site commits its pointers after this has returned 0.
template <class Pieces, class Check, class Alloc, class Layout>
int carve_first_call(Check&& check_capture, Alloc&& alloc, const char* what, Pieces* out, Layout&& lay,
                     CarveSizes* sizes = nullptr) {
  if (what && check_capture(what)) return 1;
  Pieces pieces{};
  Carver measure(nullptr, 0);
  lay(measure, pieces);
  void* block = nullptr;
  if (alloc(&block, measure.off)) return 1;
  Carver place(block, measure.off);
  lay(place, pieces);
  *out = pieces;
  if (sizes) *sizes = CarveSizes{place.off, place.payload};
  return 0;
}

}  // namespace jh
