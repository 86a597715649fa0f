// staging_main.cpp -- the control flow of nad::StagingBuffer (neural_amd/csrc/staging.h) against counting stubs, no
// HIP device: every order of failure, through finish() and through the destructor alone.  Built with
// -fsanitize=address,undefined and run by tests/test_staging_cpu.py; the buffer is a real heap block, so a double
// free, a leak or a use after free is the sanitizer's to report.  Exit status 0 and "staging ok" when every case holds.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../neural_amd/csrc/staging.h"

namespace {

std::vector<std::string> g_log;          // "malloc", "sync", "free" in the order they happened
int g_fail_malloc, g_fail_sync, g_fail_free;  // the error each stub returns (0: succeeds)
int g_live;                              // blocks allocated and not yet freed

struct StubApi {
  using Error = int;
  using Stream = int;
  static constexpr Error kOk = 0;
  static Error malloc(void** p, size_t bytes) {
    g_log.push_back("malloc");
    if (g_fail_malloc) return g_fail_malloc;
    *p = std::malloc(bytes);
    g_live++;
    return kOk;
  }
  static Error sync(Stream) {
    g_log.push_back("sync");
    return g_fail_sync;
  }
  static Error free(void* p) {
    g_log.push_back("free");
    std::free(p);  // freed even when the stub reports an error: the error is about the report, not the block
    g_live--;
    return g_fail_free;
  }
};
using Staging = nad::StagingBuffer<StubApi>;

int g_bad;
void expect(bool ok, const char* name, const char* what) {
  if (!ok) {
    g_bad++;
    std::string log;
    for (const auto& s : g_log) log += s + " ";
    std::fprintf(stderr, "FAIL %s: %s (log: %s)\n", name, what, log.c_str());
  }
}
int count(const char* ev) {
  int c = 0;
  for (const auto& s : g_log) c += s == ev;
  return c;
}
int pos(const char* ev) {
  for (size_t i = 0; i < g_log.size(); i++)
    if (g_log[i] == ev) return int(i);
  return -1;
}

// one load: allocate, copy, launch, then finish() -- or, with early_return, leave as HIP_OK does and let the
// destructor clean up.  Errors: 1 malloc, 2 copy, 3 launch, 4 sync, 5 free.
struct Case {
  const char* name;
  int malloc_e, copy_e, launch_e, sync_e, free_e;
  int want;                // the error finish() must report
  const char* want_what;   // and the step it must name
};

void run_case(const Case& c, bool early_return) {
  g_log.clear();
  g_fail_malloc = c.malloc_e;
  g_fail_sync = c.sync_e;
  g_fail_free = c.free_e;
  int steps_run = 0, reported = -1;
  std::string what;
  {
    Staging s(7);
    bool ok = s.alloc(64);
    if (ok) s.ptr()[63] = 1;  // the block is writable
    ok = s.run("copy", [&] { steps_run++; return c.copy_e; });
    if (!(early_return && !ok)) {
      ok = s.run("launch", [&] { steps_run++; return c.launch_e; });
      if (!(early_return && !ok)) {
        reported = s.finish();
        what = s.what();
        expect(s.finish() == reported, c.name, "a second finish() reports the same error");
      }
    }
  }  // destructor
  const bool allocated = c.malloc_e == 0;
  expect(count("malloc") == 1, c.name, "one allocation");
  expect(count("sync") == 1, c.name, "exactly one synchronise, after failures too");
  expect(count("free") == (allocated ? 1 : 0), c.name, "freed exactly once (never when the allocation failed)");
  expect(!allocated || pos("sync") < pos("free"), c.name, "the synchronise comes before the free");
  expect(g_live == 0, c.name, "nothing left allocated");
  const int want_steps = c.malloc_e ? 0 : (c.copy_e ? 1 : 2);
  expect(steps_run == want_steps, c.name, "steps after the first failure are skipped");
  if (reported != -1) {
    expect(reported == c.want, c.name, "finish() reports the first error");
    expect(what == c.want_what, c.name, "and names the step that failed first");
  }
}

}  // namespace

int main() {
  const Case cases[] = {
      {"all succeed", 0, 0, 0, 0, 0, 0, ""},
      {"allocation fails", 1, 0, 0, 0, 0, 1, "hipMalloc of the staging buffer"},
      {"copy fails", 0, 2, 0, 0, 0, 2, "copy"},
      {"launch fails", 0, 0, 3, 0, 0, 3, "launch"},
      {"sync fails", 0, 0, 0, 4, 0, 4, "hipStreamSynchronize"},
      {"free fails", 0, 0, 0, 0, 5, 5, "hipFree of the staging buffer"},
      {"copy and sync and free fail", 0, 2, 0, 4, 5, 2, "copy"},
      {"launch and sync fail", 0, 0, 3, 4, 0, 3, "launch"},
      {"sync and free fail", 0, 0, 0, 4, 5, 4, "hipStreamSynchronize"},
      {"allocation and sync fail", 1, 0, 0, 4, 0, 1, "hipMalloc of the staging buffer"},
  };
  for (const Case& c : cases) {
    run_case(c, false);  // through finish()
    run_case(c, true);   // an early return at the first failing step: the destructor alone
  }
  if (g_bad) return 1;
  std::puts("staging ok");
  return 0;
}
