// staged_call.h -- the two call shapes shared by the C-ABI objects whose slot form uploads host-built descriptors:
// staged_call (one slot / batch call on the caller's stream) and host_call (the host form around it).
#pragma once

#include "srsran_amd/ldpc.h"

#include "api_common.h"
#include "device_buffer.h"
#include <mutex>

namespace srs_amd {

// One slot-form call: makes the device current, grows the descriptor buffer, takes the next pinned staging buffer and
// orders the call after the object's previous one (stream_order::begin).  The site then fills host(), upload()s it,
// launches, and returns finish(): the call is closed (call_scope) there, or by the destructor on an early return.
// Scratch other than the descriptor buffer is grown by the site before it opens the call.
struct staged_call {
  // `device` for a site that made the device current itself to grow other scratch first
  static constexpr int DEVICE_IS_CURRENT = -1;
  const char*   name; // of the object, for the error messages
  pinned_stage& stage;
  hipStream_t   s;
  hipError_t    e;
  call_scope    scope;
  staged_call(const char*    object_name,
              int            device,
              device_buffer& descriptors,
              size_t         device_bytes,
              pinned_stage&  st,
              size_t         staged_bytes,
              stream_order&  order,
              hipStream_t    stream,
              stream_fan*    fan = nullptr) :
    name(object_name),
    stage(st),
    s(stream),
    e(device == DEVICE_IS_CURRENT ? hipSuccess : hipSetDevice(device)),
    scope(order, fan, stream)
  {
    if (e == hipSuccess) {
      e = descriptors.ensure(device_bytes);
    }
    if (e == hipSuccess) {
      e = stage.acquire(staged_bytes);
    }
    if (e == hipSuccess) {
      e = order.begin(s);
    }
    scope.open = e == hipSuccess; // nothing to close when the call never began
  }
  // false: the call did not begin (host() is not writable); the site returns finish()
  bool ok() const { return scope.open; }
  // the pinned staging buffer, writable until upload()
  template <typename T = unsigned char>
  T* host(size_t offset = 0) const
  {
    return stage.at<T>(offset);
  }
  // the first n staged bytes to device memory dst on the call's stream
  hipError_t upload(void* dst, size_t n) { return e = stage.upload(dst, n, s); }
  // Closes the call and returns its first failure: the prologue or upload, the site's launches, a nested C-ABI call
  // of the site (rc, its message already recorded), the completion event.
  int finish(hipError_t launches = hipSuccess, int rc = SRS_AMD_OK)
  {
    if (!scope.open) {
      return fail(SRS_AMD_EHIP, "%s scratch: %s", name, hipGetErrorString(e));
    }
    e = e != hipSuccess ? e : launches;
    if (e != hipSuccess) {
      rc = fail(SRS_AMD_EHIP, "%s launch: %s", name, hipGetErrorString(e));
    }
    const hipError_t done = scope.close();
    if (rc == SRS_AMD_OK && done != hipSuccess) {
      rc = fail(SRS_AMD_EHIP, "%s completion event: %s", name, hipGetErrorString(done));
    }
    return rc;
  }
};

// One host-form call, serialised per object by host_mtx for its whole length: grow() the private device buffers,
// in() the inputs, run the slot form with one item on stream(), out() the results, return finish(rc).  Every copy is
// queued on the object's private stream, and finish() waits for that stream on every path, so no copy from or to the
// caller's memory is pending when the call returns and no other host call's input can reach this call's kernels.
struct host_call {
  std::lock_guard<std::mutex> lock;
  const char*                 name;
  hipStream_t                 s;
  hipError_t                  e;
  host_call(const char* object_name, std::mutex& host_mtx, int device, hipStream_t stream) :
    lock(host_mtx), name(object_name), s(stream), e(hipSetDevice(device))
  {
  }
  bool ok() const { return e == hipSuccess; }
  void grow(device_buffer& b, size_t n)
  {
    if (e == hipSuccess) {
      e = b.ensure(n);
    }
  }
  void in(void* device, const void* host, size_t n) { copy(device, host, n, hipMemcpyHostToDevice); }
  void out(void* host, const void* device, size_t n) { copy(host, device, n, hipMemcpyDeviceToHost); }
  // rc: what the slot form returned (SRS_AMD_OK when it was not reached)
  int finish(int rc = SRS_AMD_OK)
  {
    const hipError_t sync = hipStreamSynchronize(s);
    if (rc != SRS_AMD_OK) {
      return rc;
    }
    e = e != hipSuccess ? e : sync;
    return e == hipSuccess ? SRS_AMD_OK : fail(SRS_AMD_EHIP, "%s host transfer: %s", name, hipGetErrorString(e));
  }

private:
  void copy(void* dst, const void* src, size_t n, hipMemcpyKind kind)
  {
    if (e == hipSuccess && n != 0) {
      e = hipMemcpyAsync(dst, src, n, kind, s);
    }
  }
};

} // namespace srs_amd
