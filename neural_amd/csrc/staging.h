// staging.h -- a device staging buffer bound to a stream: allocate, run the steps that use it, then synchronise the
// stream and free -- in that order on every way out, so no exit leaves the buffer allocated or a copy in flight that
// still reads host memory.  The first step that fails is kept by name; later steps are skipped.
//
// Api supplies the runtime (capi_internal.h binds HIP; tests/staging_main.cpp binds counting stubs):
//   Error, Stream, kOk, malloc(void**, size_t), sync(Stream), free(void*)
#pragma once
#include <cstddef>
#include <cstdint>

namespace nad {

template <class Api>
class StagingBuffer {
 public:
  using Error = typename Api::Error;
  explicit StagingBuffer(typename Api::Stream st) : st_(st) {}
  StagingBuffer(const StagingBuffer&) = delete;
  StagingBuffer& operator=(const StagingBuffer&) = delete;
  ~StagingBuffer() { (void)finish(); }  // a return before finish(): the same sync, then free, silently

  bool alloc(size_t bytes) {
    return run("hipMalloc of the staging buffer", [&] { return Api::malloc(&p_, bytes); });
  }
  uint8_t* ptr() const { return static_cast<uint8_t*>(p_); }

  // fn() unless a step has failed already; the first failure and its name are kept.  True while nothing has failed
  template <class F>
  bool run(const char* what, F&& fn) {
    if (e_ == Api::kOk) note(what, fn());
    return e_ == Api::kOk;
  }

  // synchronise (also after a failure: a copy may still read the caller's memory), then free; once
  Error finish() {
    if (!done_) {
      done_ = true;
      note("hipStreamSynchronize", Api::sync(st_));
      if (p_) note("hipFree of the staging buffer", Api::free(p_));
      p_ = nullptr;
    }
    return e_;
  }
  Error error() const { return e_; }
  const char* what() const { return what_; }  // the step that failed first

 private:
  void note(const char* what, Error e) {
    if (e_ == Api::kOk && e != Api::kOk) {
      e_ = e;
      what_ = what;
    }
  }
  typename Api::Stream st_;
  void* p_ = nullptr;
  Error e_ = Api::kOk;
  const char* what_ = "";
  bool done_ = false;
};

}  // namespace nad
