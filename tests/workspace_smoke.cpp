// A host-only program over jarvis-hybridnet_amd/csrc/workspace.h ALONE (no HIP header, no library): the Carver's
// measuring and placing passes agree, pieces are 256-byte aligned, ordered and disjoint, and carve_first_call -- the one
// way a predictor's first-call workspaces are made -- leaves the caller's pointers alone when the allocator fails or
// the site is inside a stream capture, where it hands back the site's own message.  Built and run by
// tests/test_native_abi.py::test_workspace_carving (g++, no hipcc).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "workspace.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "workspace_smoke.cpp:%d: %s\n", __LINE__, #cond);  \
      return 1;                                                          \
    }                                                                    \
  } while (0)

namespace {

// pieces of 1, 255, 256 and 257 bytes and a zero-count piece (between them, so that it has neighbours on both sides)
constexpr int kPieces = 5;
const size_t kBytes[kPieces] = {1, 255, 0, 256, 257};
const size_t kPadded[kPieces] = {256, 256, 0, 256, 512};
struct Pieces { char* p[kPieces]; };

void lay(jh::Carver& c, Pieces& w) {
  w.p[0] = c.take<char>(1);
  w.p[1] = c.take<char>(255);
  w.p[2] = reinterpret_cast<char*>(c.take<double>(0));
  w.p[3] = reinterpret_cast<char*>(c.take<int>(64));
  w.p[4] = c.take<char>(257);
}

int carver_passes() {
  size_t payload = 0, padded = 0;
  for (int i = 0; i < kPieces; ++i) { payload += kBytes[i]; padded += kPadded[i]; }
  // the measuring pass: every piece null, the total is what the pieces need
  jh::Carver measure(nullptr, 0);
  Pieces m;
  lay(measure, m);
  for (char* p : m.p) CHECK(p == nullptr);
  CHECK(measure.off == padded);
  CHECK(measure.payload == payload);
  // the placing pass over a block of exactly that size
  char* block = static_cast<char*>(malloc(measure.off));
  CHECK(block);
  jh::Carver place(block, measure.off);
  Pieces w;
  lay(place, w);
  CHECK(place.off == measure.off && place.fits());
  CHECK(place.payload == payload);
  size_t end = 0;                             // (where the previous piece ended)
  for (int i = 0; i < kPieces; ++i) {
    const size_t at = (size_t)(w.p[i] - block);
    CHECK(at % 256 == 0);                     // aligned relative to the base
    CHECK(at >= end);                         // in the order taken, not overlapping the piece before
    CHECK(at + kBytes[i] <= measure.off);     // ends inside the block
    end = at + kBytes[i];
    memset(w.p[i], 0xA5, kBytes[i]);          // (a sanitizer build sees every byte of every piece written)
  }
  // one byte less does not fit
  jh::Carver small(block, measure.off - 1);
  lay(small, w);
  CHECK(!small.fits());
  free(block);
  return 0;
}

// stand-ins for the predictor's allocator and capture check
struct Host {
  bool capturing = false, fail = false;
  int allocations = 0;
  const char* refused = nullptr;
  void* block = nullptr;
  size_t bytes = 0;
  int outside_capture(const char* what) {
    if (capturing) refused = what;
    return capturing ? 1 : 0;
  }
  int alloc(void** p, size_t n) {
    if (fail) return 1;
    ++allocations;
    block = *p = malloc(n);
    bytes = n;
    return block ? 0 : 1;
  }
};

int carve(Host& h, const char* what, Pieces* out, jh::CarveSizes* sizes) {
  return jh::carve_first_call([&](const char* w) { return h.outside_capture(w); },
                              [&](void** p, size_t n) { return h.alloc(p, n); }, what, out, lay, sizes);
}

int helper() {
  static const char what[] = "the first call of a site allocates its workspace: make it outside a stream capture";
  char sentinel[kPieces];
  Pieces mine;
  for (int i = 0; i < kPieces; ++i) mine.p[i] = &sentinel[i];
  const Pieces before = mine;
  jh::CarveSizes sizes{7, 9};

  Host failing;
  failing.fail = true;
  CHECK(carve(failing, what, &mine, &sizes) != 0);
  CHECK(memcmp(&mine, &before, sizeof mine) == 0 && sizes.bytes == 7 && sizes.payload == 9);
  CHECK(failing.refused == nullptr);

  Host capturing;
  capturing.capturing = true;
  CHECK(carve(capturing, what, &mine, &sizes) != 0);
  CHECK(memcmp(&mine, &before, sizeof mine) == 0 && sizes.bytes == 7 && sizes.payload == 9);
  CHECK(capturing.refused == what);           // the site's own message, handed to the check as it was given
  CHECK(capturing.allocations == 0);

  // a site without a stream skips the check (what == nullptr): the allocation is made even while "capturing"
  Host unasked;
  unasked.capturing = true;
  CHECK(carve(unasked, nullptr, &mine, &sizes) == 0);
  CHECK(unasked.refused == nullptr && unasked.allocations == 1);
  free(unasked.block);

  Host ok;
  CHECK(carve(ok, what, &mine, &sizes) == 0);
  CHECK(ok.allocations == 1);                 // ONE allocation, of the measured size
  CHECK(sizes.bytes == ok.bytes && sizes.bytes == 256 + 256 + 0 + 256 + 512);
  CHECK(sizes.payload == 1 + 255 + 0 + 256 + 257);   // the unpadded sum
  CHECK(mine.p[0] == ok.block);
  for (int i = 0; i < kPieces; ++i) {
    CHECK(mine.p[i] >= static_cast<char*>(ok.block));
    CHECK(mine.p[i] + kBytes[i] <= static_cast<char*>(ok.block) + ok.bytes);
    memset(mine.p[i], 0x5A, kBytes[i]);
  }
  free(ok.block);
  return 0;
}

}  // namespace

int main() {
  if (carver_passes() || helper()) return 1;
  printf("workspace ok\n");
  return 0;
}
