// nbx_analysis.hpp -- the host side that the analysis calls and the two Hermite steppers share on top of nbx_object.hpp and
// nbx_batch.hpp: scratch that grows and never shrinks, the bodies of a range of members and the words of its size bound, a
// ragged ensemble's member table and grid extents, and the enqueue / read back / synchronise skeleton.  Host-only: it defines
// no kernel and includes no kernel header, so every translation unit keeps compiling exactly the kernels it includes itself,
// and it names no scratch field of any call: a caller hands in the addresses of its own.  Not part of the C-ABI.
//
// What stays with each call: its member struct (a kernel argument type) and the maker that fills one, its launches, its check
// sequence and error texts, and any flow that is not "enqueue, one copy back, one synchronisation".
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "nbx_ensemble_internal.hpp"  // struct nbx_ensemble; nbx_batch.hpp: device_table, MemberSpan
#include "nbx_field_shape.hpp"        // field_shape: the launch-shape rule of every call served here
#include "nbx_ragged_internal.hpp"    // struct nbx_ragged

// Nothing of this layer is visible outside the library, as nbx_batch.hpp.
#pragma GCC visibility push(hidden)
namespace nbx_detail {

// *p holds at least `bytes`: allocated on first use, replaced by a larger buffer -- never a smaller one -- when a call needs more
inline int ensure_bytes(void** p, size_t* cap, size_t bytes, const char* where, const char* what) {
  if (*p && *cap >= bytes) return NBX_OK;
  if (*p) HIP_TRY(hipFree(*p));
  *p = nullptr;
  *cap = 0;
  char* dev = nullptr;
  const int rc = device_alloc(&dev, bytes, where, what);
  if (rc) return rc;
  *p = dev;
  *cap = bytes;
  return NBX_OK;
}

// the bodies of members [first, first + count), and the words of the error text that bounds them
inline long long range_bodies(const nbx_ensemble* e, int, int count) { return (long long)count * e->n; }
inline long long range_bodies(const nbx_ragged* r, int first, int count) {
  long long total = 0;
  for (int k = first; k < first + count; ++k) total += r->layout(k).n;
  return total;
}
inline const char* range_noun(const nbx_ensemble*) { return "count * n exceeds"; }
inline const char* range_noun(const nbx_ragged*) { return "the bodies of the range exceed"; }

// the same of the whole object, for the calls that take no range
inline long long object_bodies(const nbx_ensemble* e) { return range_bodies(e, 0, e->members); }
inline long long object_bodies(const nbx_ragged* r) { return range_bodies(r, 0, r->members); }
inline const char* bodies_noun(const nbx_ensemble*) { return "members * n exceeds"; }
inline const char* bodies_noun(const nbx_ragged*) { return "the bodies of the members exceed"; }

// A ragged ensemble's member table, built and put on the device by the first call and kept for the object's life: nothing
// happens once *slot is set.  Entry k is make(layout(k), out_off), out_off the bodies of the members before k.  `src` receives
// the host entries, which the copy reads asynchronously: the caller keeps them until it has synchronised (a local vector of
// Member), or with the object if it never does (the object's vector of char).
template <typename Member, typename Elem, typename Make>
int ragged_member_table(nbx_ragged* r, void** slot, std::vector<Elem>* src, const char* where, Make make) {
  static_assert(sizeof(Member) % sizeof(Elem) == 0, "src holds whole entries: its elements are Member or bytes");
  if (*slot) return NBX_OK;
  src->resize(sizeof(Member) / sizeof(Elem) * (size_t)r->members);
  char* const bytes = (char*)src->data();
  unsigned long long out_off = 0;
  for (int k = 0; k < r->members; ++k) {
    const MemberSpan mem = r->layout(k);
    const Member entry = make(mem, out_off);
    std::memcpy(bytes + sizeof(Member) * (size_t)k, &entry, sizeof(Member));
    out_off += (unsigned long long)mem.n;
  }
  Elem* dev = nullptr;
  const int rc = device_table(r, &dev, *src, where, "the member table");
  if (rc) return rc;
  *slot = dev;
  return NBX_OK;
}

// The x and y extents of a ragged launch over members [first, first + count): the largest number of columns and of splits of
// field_shape(points, n) any of them has, a member's workgroups beyond its own return at once.  points is the member's n
// (m == 0: the call works at the bodies) or the caller's m points per member.
struct GridExtents {
  int columns, splits;
};
inline GridExtents ragged_extents(const nbx_ragged* r, int first, int count, int m = 0) {
  GridExtents g{1, 1};
  for (int k = first; k < first + count; ++k) {
    const int n = r->layout(k).n;
    const nbx::FieldShape s = nbx::field_shape(m ? m : n, n);
    g.columns = std::max(g.columns, s.columns);
    g.splits = std::max(g.splits, s.splits);
  }
  return g;
}

// enqueue() -- the caller's copies in and launches on o->stream, an int that may come from HIP_TRY -- then `bytes` from `dev` to
// `host` and one synchronisation.  On any failure the stream is drained before the error is returned: no copy may outlive the
// host buffers of the caller.
template <typename Enqueue>
int read_back(Object* o, void* host, const void* dev, size_t bytes, Enqueue enqueue) {
  const int rc = [&]() -> int {
    const int rc_enqueue = enqueue();
    if (rc_enqueue) return rc_enqueue;
    HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return NBX_OK;
  }();
  if (rc) (void)hipStreamSynchronize(o->stream);
  return rc;
}

}  // namespace nbx_detail
#pragma GCC visibility pop
