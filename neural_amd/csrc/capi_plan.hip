// capi_plan.hip -- the dense dry runs (include/neural_amd.h): what a forward, a fused QKV, a fused gate/up, a batch or
// a row gather would launch, no GPU needed.  Each entry is its argument check, then the exported forward entry itself
// on stand-in arguments under the launch recorder (capi_internal.h: dry_run6, stand_in, plan_weight_geometry): every
// launch statement on that path goes through planned(), so the stand-ins are never dereferenced.  The record is the
// last main launch (kernel, grid, block, ksplit, fold) and the count of all launches.
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace nad;

namespace {
bool args_ok(const char* family, const int64_t* out, int nout, int m) {
  if (out && nout >= 0 && m > 0) return true;
  set_err("%s: bad arguments (m=%d)", family, m);
  return false;
}

// the scalar entries' weights: integer formats only; a group size <= 0 is one group per channel
bool scalar_bits(int bits) { return bits == 2 || bits == 4 || bits == 8; }
void scalar_weight(DeviceWeight& w, int i, int bits, int n, int k, int blocksize, int scale_t, int asym) {
  plan_weight_geometry(w, bits, n, k, blocksize <= 0 ? k : blocksize, scale_t, asym, 0);
  plan_weight_assign(w, i);
}

// a loaded or a geometry-only (nad_weight_plan_only) weight for the dry runs of fused calls: nothing is launched on it
const DeviceWeight* plan_weight(const void* p) {
  const auto* w = static_cast<const DeviceWeight*>(p);
  if (w && w->magic == kWeightMagic) return w;
  set_err("nad_plan_*: weight descriptor is not a neural_amd device weight");
  return nullptr;
}

int plan_for(const DeviceWeight& w, int m, int act_dtype, int64_t* out, int nout) {
  if (!args_ok("nad_plan_*", out, nout, m)) return -1;
  return dry_run6(out, nout, [&] {
    return nad_device_forward(stand_in<const void>(kStandAct), act_dtype, &w, stand_in<float>(kStandOut), m, w.n, w.k,
                              w.k, w.n, kEpiNone, nullptr, 0, nullptr, 0, nullptr);
  });
}

int plan_qkv_for(const DeviceWeight* const ws[3], int m, int act_dtype, int64_t* out, int nout) {
  if (!args_ok("nad_plan_qkv*", out, nout, m)) return -1;
  const int k = ws[0]->k;
  return dry_run6(out, nout, [&] {
    return nad_device_qkv_forward(stand_in<const void>(kStandAct), act_dtype, ws[0], ws[1], ws[2],
                                  stand_in<float>(kStandOut, 0), stand_in<float>(kStandOut, 1),
                                  stand_in<float>(kStandOut, 2), m, k, k, ws[0]->n, ws[1]->n, ws[2]->n, nullptr);
  });
}

// SiLU * mul, with the tmp1 output
int plan_gate_up_for(const DeviceWeight& w1, const DeviceWeight& w3, int m, int act_dtype, int64_t* out, int nout) {
  if (!args_ok("nad_plan_gate_up*", out, nout, m)) return -1;
  return dry_run6(out, nout, [&] {
    return nad_device_ffn_gate_up(stand_in<const void>(kStandAct), act_dtype, &w1, &w3, stand_in<float>(kStandOut, 0),
                                  stand_in<float>(kStandOut, 1), m, w1.k, w1.n, w1.k, kEpiSiluMul, nullptr);
  });
}
}  // namespace

extern "C" int nad_plan_forward(int bits, int n, int k, int blocksize, int scale_t, int asym, int m, int act_dtype,
                                int64_t* out, int nout) {
  if (!scalar_bits(bits) || n <= 0 || k <= 0) {
    set_err("nad_plan_forward: bad arguments (bits=%d n=%d k=%d)", bits, n, k);
    return -1;
  }
  DeviceWeight w;
  scalar_weight(w, 0, bits, n, k, blocksize, scale_t, asym);
  return plan_for(w, m, act_dtype, out, nout);
}

// as_weight runs before the recording starts, so it refuses a geometry-only descriptor here as it does for a launch:
// this entry is for loaded weights (the scalar entry above and the fused entries below take the others)
extern "C" int nad_plan_weight(const void* devstor, int m, int act_dtype, int64_t* out, int nout) {
  const DeviceWeight* w = as_weight(devstor);
  return w ? plan_for(*w, m, act_dtype, out, nout) : -1;
}

extern "C" int nad_plan_qkv_forward(int bits, int nq, int nk, int nv, int k, int blocksize, int scale_t, int asym,
                                    int m, int act_dtype, int64_t* out, int nout) {
  if (!scalar_bits(bits) || nq <= 0 || nk <= 0 || nv <= 0 || k <= 0) {
    set_err("nad_plan_qkv_forward: bad arguments (bits=%d n=%d,%d,%d k=%d)", bits, nq, nk, nv, k);
    return -1;
  }
  const int ns[3] = {nq, nk, nv};
  DeviceWeight w[3];
  for (int i = 0; i < 3; i++) scalar_weight(w[i], i, bits, ns[i], k, blocksize, scale_t, asym);
  const DeviceWeight* ws[3] = {&w[0], &w[1], &w[2]};
  return plan_qkv_for(ws, m, act_dtype, out, nout);
}

extern "C" int nad_plan_qkv(const void* wq, const void* wk, const void* wv, int m, int act_dtype, int64_t* out,
                            int nout) {
  const DeviceWeight* ws[3] = {plan_weight(wq), plan_weight(wk), plan_weight(wv)};
  if (!ws[0] || !ws[1] || !ws[2]) return -1;
  return plan_qkv_for(ws, m, act_dtype, out, nout);
}

extern "C" int nad_plan_gate_up_forward(int bits, int n, int k, int blocksize, int scale_t, int asym, int m,
                                        int act_dtype, int64_t* out, int nout) {
  if (!scalar_bits(bits) || n <= 0 || k <= 0) {
    set_err("nad_plan_gate_up_forward: bad arguments (bits=%d n=%d k=%d)", bits, n, k);
    return -1;
  }
  DeviceWeight w[2];
  for (int i = 0; i < 2; i++) scalar_weight(w[i], i, bits, n, k, blocksize, scale_t, asym);
  return plan_gate_up_for(w[0], w[1], m, act_dtype, out, nout);
}

extern "C" int nad_plan_gate_up(const void* w1p, const void* w3p, int m, int act_dtype, int64_t* out, int nout) {
  const DeviceWeight* w1 = plan_weight(w1p);
  const DeviceWeight* w3 = plan_weight(w3p);
  if (!w1 || !w3) return -1;
  return plan_gate_up_for(*w1, *w3, m, act_dtype, out, nout);
}

// nad_batch_run (the batched launch has no specialised or load-ahead form), the instantiation named by
// launch_gemv_batch's own launch statement
extern "C" int nad_plan_batch(void* batch, int64_t* out, int nout) {
  if (!batch || !out || nout < 0) {
    set_err("nad_plan_batch: bad arguments");
    return -1;
  }
  return dry_run6(out, nout, [&] { return nad_batch_run(batch, nullptr); });
}

// The same for n problems on a loaded or geometry-only weight: the batch is created without its device table
// (nad_batch_create under the recorder), recorded and destroyed.
extern "C" int nad_plan_batch_only(const void* devstor, int n, int64_t* out, int nout) {
  if (!devstor || n <= 0 || !out || nout < 0) {
    set_err("nad_plan_batch_only: bad arguments");
    return -1;
  }
  const std::vector<nad_batch_problem> p(
      static_cast<size_t>(n), nad_batch_problem{devstor, stand_in<const float>(kStandAct), stand_in<float>(kStandOut)});
  return dry_run6(out, nout, [&] {
    void* b = nad_batch_create(p.data(), n);
    const int rc = b ? nad_batch_run(b, nullptr) : -1;
    nad_batch_destroy(b);
    return rc;
  });
}

extern "C" int nad_plan_get_rows(const void* devstor, int m, int out_dtype, int64_t* out, int nout) {
  const char* who = "nad_plan_get_rows";
  if (!out || nout < 0) {
    set_err("%s: no output buffer", who);
    return -1;
  }
  const DeviceWeight* w = any_weight(who, devstor);
  if (!w) return -1;
  const int ldo = (w->k + 7) & ~7;
  return dry_run6(out, nout, [&] {
    return get_rows(who, devstor, nullptr, 1, m, stand_in<void>(kStandOut), out_dtype, ldo, nullptr);
  });
}

// The geometry-only descriptor the dry runs take without a GPU: no section pointers, which is what marks it as holding
// no weights.
extern "C" int nad_weight_plan_only(int bits, int n, int k, int blocksize, int scale_t, int asym, int act_order,
                                    void* devstor) {
  const char* who = "nad_weight_plan_only";
  if (!devstor || !plan_geometry_ok(bits, n, k, scale_t)) {
    set_err("%s: bad geometry (bits=%d n=%d k=%d scale=%d)", who, bits, n, k, scale_t);
    return -1;
  }
  if (blocksize <= 0 || blocksize > k) blocksize = k;
  if (bits != 6 && blocksize % 32 && blocksize < k) {
    set_err("%s: group size must be a multiple of 32", who);
    return -1;
  }
  DeviceWeight w;
  plan_weight_geometry(w, bits, n, k, blocksize, scale_t, asym, act_order);
  std::memcpy(devstor, &w, sizeof(w));
  return 0;
}
