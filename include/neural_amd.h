/*
 * neural_amd.h -- C ABI of the MI355X-native weight-only-quantized (WOQ) matmul core.
 *
 * Drop-in for the BesTLA boundary of Neural Speed (hoivb612/neural).  Every entry point below keeps the name,
 * argument meaning and error behaviour of the reference interface it replaces (cited per group; paths relative to
 * the reference repo root).  Plain C types only: no torch, no HIP types (a HIP stream is passed as void* "queue").
 *
 * Build: `make -C neural_amd` -> neural_amd/libneural_amd.so (gfx950).  Link it in place of
 * neural_speed/core/layers/ne_bestla.cpp + ne_bestla_sycl.cpp + bestla_gemm.cpp.
 *
 * Errors: bool/int functions return false/nonzero; void functions (whose reference counterparts assert(0) or are
 * silently skipped, e.g. bestla_gemm.cpp:542-590) print "neural_amd: <reason>" to stderr and record it; read it with
 * nad_last_error().  Nothing is silently skipped.
 */
#ifndef NEURAL_AMD_H
#define NEURAL_AMD_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ===== device half: neural_speed/core/ne_bestla.h:85-112 (implemented for SYCL in
 * neural_speed/core/layers/ne_bestla_sycl.cpp:25-171).  queue == hipStream_t; device == NadDevice*. */
void* bestla_create_device(bool profile);               /* ne_bestla.h:86 */
void* bestla_get_device_queue(void* device);            /* ne_bestla.h:87 */
void bestla_release_device(void* device);               /* ne_bestla.h:88 */
size_t bestla_device_gmem_size(void* device);           /* ne_bestla.h:89 */
void* bestla_device_malloc(size_t size, void* queue);   /* ne_bestla.h:90 */
void bestla_device_free(void* ptr, void* queue);        /* ne_bestla.h:91 */
void bestla_device_memcpy(void* dstptr, const void* srcptr, size_t size, void* queue);      /* ne_bestla.h:92 */
void bestla_device_memcpy_sync(void* dstptr, const void* srcptr, size_t size, void* queue); /* ne_bestla.h:93 */
void bestla_device_sync(void* queue);                   /* ne_bestla.h:94 */
/* size of the per-tensor device descriptor embedded after ne_tensor (ne_layers.c:946-949) */
size_t bestla_device_storage_size(void);                /* ne_bestla.h:95 */
/* parse a host BTLA blob, repack it on the GPU into the MFMA tile layout inside `deviceptr` (which the caller sized
 * with the blob's byte size, model_files.h:1515-1525) and fill the host descriptor `devstor`. */
void bestla_device_load_storage(void* hoststor, void* devstor, void* deviceptr, void* queue); /* ne_bestla.h:96 */
/* Y[m][n] = X[m][k] . W^T, X/Y fp32 device pointers (row strides lda/ldo in elements), asynchronous on queue */
void bestla_device_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k, int lda,
                                  int ldo, void* workspace, void* queue); /* ne_bestla.h:97-98 */

/* ===== host half: neural_speed/core/ne_bestla.h:21-83 (CPU implementation: core/layers/inner_product.cpp,
 * ip_fusion_qkv.cpp, ip_fusion_ffn.cpp, ne_bestla.cpp).  Same host-pointer contract; the work runs on the GPU
 * (weights uploaded once per blob and cached, activations/outputs staged over PCIe).  Pointers that are already
 * device memory are used in place. */
void bestla_init(void);                                 /* ne_bestla.h:31 */
int bestla_set_threads(int _nth);                       /* ne_bestla.h:23: host packing threads */
void* bestla_get_thread_handle(void);                   /* ne_bestla.h:25 */
unsigned long long bestla_f32f32_get_workspace_size(int _m, int _n, int _k, void* wptr); /* ne_bestla.h:33 */
void bestla_f32f32_forward(float* activation, void* weiptr, float* output, int _m, int _n, int _k, int lda, int ldo,
                           void* workspace);            /* ne_bestla.h:35-36 */
bool bestla_fusion_add_f32f32_support(void* weiptr, int _m, int _n, int _k); /* ne_bestla.h:38 */
void bestla_fusion_add_f32f32_forward(float* activation, void* weiptr, float* bias, float* output, int _m, int _n,
                                      int _k, int lda, int ldo, bool boardcast_bias, void* workspace); /* :39-40 */
unsigned long long bestla_fusion_QKV_f32f32_get_workspace_size(int _m, int _n, int _k, void* w1ptr); /* :42 */
bool bestla_fusion_QKV_f32f32_support(void* wqptr, void* wkptr, void* wvptr, int _m, int _n, int _k); /* :44 */
void bestla_fusion_QKV_f32f32_forward(float* activation, void* wqptr, void* wkptr, void* wvptr, float* output, int _m,
                                      int _n, int _k, int lda, int ldo, void* workspace); /* :46-47 */
unsigned long long bestla_fusion_FFN_f32f32_get_workspace_size(int seq, int fin, int fmid, int fout, void* w1ptr,
                                                               void* w2ptr); /* :49-50 */
bool bestla_fusion_FFN_SiLu_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin, int fmid,
                                           int fout); /* :57 */
void bestla_fusion_FFN_SiLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr, float* tmp1,
                                           float* tmp2, float* output, int seq, int fin, int fmid, int fout,
                                           void* workspace); /* :58-60 */
bool bestla_fusion_FFN_Gelu_Mul_f32f32_support(void* w1ptr, void* w2ptr, void* w3ptr, int seq, int fin, int fmid,
                                               int fout); /* :52-53 */
void bestla_fusion_FFN_Gelu_Mul_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, void* w3ptr, float* tmp1,
                                               float* tmp2, float* output, int seq, int fin, int fmid, int fout,
                                               void* workspace); /* :54-56 */
bool bestla_fusion_FFN_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid, int fout); /* :62 */
void bestla_fusion_FFN_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* tmp1, float* output,
                                           int seq, int fin, int fmid, int fout, void* workspace); /* :63-64 */
bool bestla_fusion_FFN_Add_GeLu_f32f32_support(void* w1ptr, void* w2ptr, int seq, int fin, int fmid,
                                               int fout); /* :66 */
void bestla_fusion_FFN_Add_GeLu_f32f32_forward(float* activation, void* w1ptr, void* w2ptr, float* b1ptr,
                                               float* b2ptr, float* tmp1, float* output, int seq, int fin, int fmid,
                                               int fout, bool boardcast_bias, void* workspace); /* :67-69 */
void bestla_unpackweight_fp32(void* wptr, int n, int k, float* fp32data, int ld); /* ne_bestla.h:71 */
void bestla_packweight_copyattr(const float* f32ptr, void* dstpr, int n, int k, int ld, void* srcptr); /* :73 */

/* ===== pack / format API: neural_speed/core/layers/bestla_gemm.h:30-58 (C++ linkage in the reference; C here).
 * QuantType/ScaleDtype are BTLA_DTYPE values (bestla/bestla/bestla.h:38-87), CompType is ne_comp_type
 * (core/data_types.h:57-63).  The core layout is chosen for an emulated host ISA (NAD_HOST_ISA, default
 * Sapphire Rapids) exactly as BTLAGemmPackBSizeLocal does (bestla_gemm.cpp:241-300). ThreadPool may be NULL. */
typedef struct BTLA_GEMM_DATA_PACKED_PARAMS {
  const float* A; /* address of A (float32 matrix) */
  const void* B;  /* address of B (packed nbits blob) */
  float* C;       /* address of result matrix */
  int lda;        /* leading dimension of A */
  int ldc;        /* leading dimension of C */
} BTLA_GEMM_DATA_PACKED_PARAMS;     /* bestla_gemm.h:30-36 */
size_t BTLAGemmPackBSize(size_t N, size_t K, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype, bool isAsym,
                         int CompType, int* shuffle_indice); /* bestla_gemm.h:38-39 */
bool BTLAGemmQuantPackB(void* PackedBuf, const float* FpData, size_t N, size_t K, size_t ldb, size_t BlkSize,
                        uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType, bool isTrans,
                        void* ThreadPool); /* bestla_gemm.h:41-43 */
bool BTLAGemmPackB(void* PackedBuf, const int8_t* QData, const float* Scales, const int8_t* Zp, size_t N, size_t K,
                   size_t ldb, size_t BlkSize, uint32_t QuantType, uint32_t ScaleDtype, bool isAsym, int CompType,
                   int* shuffle_indice, void* ThreadPool); /* bestla_gemm.h:48-50 */
bool BTLAGemmUnPackB(float* FpData, const void* PackedBuf, size_t N, size_t K, size_t ldb,
                     void* ThreadPool); /* bestla_gemm.h:52 */
bool BTLAGemmBatchDriver(const size_t M, const size_t N, const size_t K, const size_t BatchN,
                         const BTLA_GEMM_DATA_PACKED_PARAMS* DataParams, int8_t* WorkSpace,
                         void* ThreadPool); /* bestla_gemm.h:54-55 */

/* ===== tensor-parallel communicator: neural_speed/core/parallel_context.h:21-48 (oneCCL/MPI + SHM in the reference,
 * parallel_context.cpp:19-159, shared_memory_ccl.hpp:100-139).  Implemented in csrc/parallel_context.hip: TCP
 * rendezvous from RANK/WORLD_SIZE (or OMPI_/PMI_ env), RCCL on a context stream for device buffers, a one-shot IPC
 * peer-buffer all-reduce for small device messages, host buffers staged through the device (or carried over the
 * rendezvous sockets when no GPU is present).  `count` is an element count (the reference passes byte counts at
 * ne_layers.c:5474 -- callers of this library pass elements). */
typedef struct parallel_context parallel_context;
parallel_context* init_parallel_context(void);   /* parallel_context.h:40 (process-wide singleton) */
int get_tp_size(parallel_context* p);             /* :41 */
int get_tp_rank(parallel_context* p);             /* :42 */
bool is_master(parallel_context* p);              /* :43 */
void barrier(parallel_context* p);                /* :44 (also drains this rank's device work) */
void broadcast(parallel_context* p, float* buffer, size_t count);                           /* :45, root 0 */
void alltoall(parallel_context* p, float* send_buffer, float* recv_buffer, size_t count);   /* :46, count per rank */
void reduce_add(parallel_context* p, float* send_buffer, float* recv_buffer, size_t count); /* :47, sum */
/* native: sum all-reduce of device buffers on `stream` (a hipStream_t; NULL = the null stream, as everywhere in this
 * library), asynchronous, graph-capturable */
int nad_pc_allreduce_f32(parallel_context* p, const float* send, float* recv, size_t count, void* stream);
int nad_pc_set_stream(parallel_context* p, void* stream);   /* stream of the reference entry points (default NULL) */
double nad_pc_max_f64(parallel_context* p, double v);        /* max over ranks (host value; bench timing) */
int nad_pc_status(parallel_context* p);   /* 0 ok, 1 a one-shot all-reduce gave up waiting for a peer */
int nad_pc_info(parallel_context* p);     /* bit0 GPU transport, bit1 one-shot IPC path, bit2 RCCL communicator,
                                             bit3 one-shot buffer is uncached fine-grained memory (else hipMalloc) */
const char* nad_pc_last_error(parallel_context* p);
void nad_pc_destroy(parallel_context* p);

/* ===== native extensions (no reference counterpart) */
#define NAD_ACT_F32 0
#define NAD_ACT_F16 1
#define NAD_ACT_BF16 2
/* device scale codes (nad_synthetic_weight, nad_plan_forward, nad_weight_info[8]) */
#define NAD_SCALE_F32 0
#define NAD_SCALE_BF16 1
#define NAD_SCALE_F16 2
#define NAD_EPI_NONE 0
#define NAD_EPI_BIAS 1
#define NAD_EPI_SILU_MUL 2
#define NAD_EPI_GELU_MUL 3
#define NAD_EPI_GELU 4
#define NAD_EPI_ADD_GELU 5
#define NAD_EPI_SILU 6
#define NAD_EPI_RES_ADD 7

const char* nad_last_error(void);
void nad_clear_error(void);
/* device bytes the tile layout of this blob needs (<= the blob size for every Llama/Mistral shape) */
size_t nad_device_weight_size(const void* hostblob);
/* bestla_device_load_storage with an explicit capacity check and a status return */
int nad_device_load(const void* hostblob, void* devstor, void* deviceptr, size_t capacity, void* queue);
/* ===== quantize and pack on the device: BTLAGemmQuantPackB + nad_device_load for a matrix that already sits in HBM,
 * byte-identical to that host path.  Integer weights only: qtype S4_CLIP, S2_CLIP or S8, sym or asym, F32 / BF16 / F16
 * scales, any CompType (the core is select_core's, so NAD_HOST_ISA picks the same one as on the host path), any group
 * size nad_device_load takes (blocksize <= 0 or >= k: per-channel; a partial last group is fine).  S1 / S3 / S5..S7,
 * F4 / F8 weights and DQ8_BNB / F8_E8M0 scales are refused by name: they stay on the host path.
 *
 * The arithmetic is quantize_kblock's sNauto branch operation for operation (fp16 / bf16 inputs are widened exactly;
 * the float -> int cast gives INT_MIN for NaN as the x86 cast does, which is how an all-zero group gets code 0 (sym) or
 * zero point 2^(bits-1) - 1 with codes -2^(bits-1) (asym)), so for every finite input the blob equals the host packer's
 * byte for byte.  For non-finite inputs the codes are unspecified; nothing faults or reads outside [n][0:k]. */
/* device bytes of the weight (== nad_device_weight_size of the blob BTLAGemmQuantPackB would write);
 * *blob_size (may be NULL) = BTLAGemmPackBSize of the same arguments; 0 + nad_last_error on refusal */
size_t nad_device_quantize_size(int n, int k, int blocksize, uint32_t qtype, uint32_t scale_dtype, int asym, int comp,
                                size_t* blob_size);
/* w: device [n][ldw] of w_dtype (the act dtype codes 0 fp32 / 1 fp16 / 2 bf16), ldw >= k.  Writes the descriptor and
 * exactly the first `bytes` of deviceptr (what nad_device_load writes of them); if blob_out != NULL also the blob --
 * header and every section, the padding of the sections as zeros -- into host memory (64-byte aligned blobs of the two
 * paths compare equal when both buffers were zero-filled: the serializer aligns relative to the base).  Errors (a null
 * pointer, ldw < k, a capacity too small -- the message states the need --, a refused dtype) are found before any
 * device work.  Synchronous, allocates its staging and frees it, like nad_device_load; not for graph capture. */
int nad_device_quantize(const void* w, int w_dtype, int n, int k, int ldw, int blocksize, uint32_t qtype,
                        uint32_t scale_dtype, int asym, int comp, void* devstor, void* deviceptr, size_t capacity,
                        void* blob_out, size_t blob_capacity, void* queue);
/* descriptor summary: [magic, bits, n, k, blocksize, ns, nt, ng, scale_t, asym, has_shuffle, bytes] */
int nad_weight_info(const void* devstor, int64_t* out12);
/* the same, versioned by the caller's buffer: writes min(n, 14) values ([12] = fold_ok: every q * scale is an fp16
 * normal, the prefill GEMM may fold the scale into the fp16 weights; [13] = the tile order, 0 stripe-major [ns][nt],
 * 1 K-major [nt][ns]), returns the number written or -1 */
int nad_weight_info2(const void* devstor, int64_t* out, int n);
/* re-read the NAD_* tuning / A-B switches from the environment (they are read once when the library loads, never per
 * call); not thread-safe against forwards running at the same time */
void nad_reload_knobs(void);
/* blob header summary (same fields as the oracle's orc_blob_info) */
int nad_blob_info(const void* hostblob, int64_t* out27);
/* Y = epi(X . W^T): X in fp32/fp16/bf16 (act_dtype), Y fp32.  bias: bias[m*bias_ld + n] (bias_ld 0 = broadcast);
 * res: residual[m*ld_res + n] for NAD_EPI_RES_ADD.  Writes exactly out[0:m, 0:n] (row stride ldo), whatever out held;
 * reads X, bias and res only inside their [m][k] / [m][n] windows.  A null bias / res for an epilogue that needs it is
 * an error (-1), found before anything else is looked at. */
int nad_device_forward(const void* act, int act_dtype, const void* devstor, float* out, int m, int n, int k, int lda,
                       int ldo, int epi, const float* bias, int bias_ld, const float* res, int ld_res, void* queue);
/* Dry run of nad_device_forward for a weight geometry (bits 2 / 4 / 8, blocksize <= 0 = per-channel, scale_t
 * NAD_SCALE_*, m rows of act_dtype): the whole host side of the call -- validation, kernel choice, geometry,
 * workspace sizing -- with every launch recorded instead of issued; no device memory is touched and no GPU is needed.
 * out (versioned by nout): [kernel NAD_KERNEL_*, grid, threads per workgroup, split-K runs, flags (bit 0: scale folded
 * into the fp16 weights; bit 1: gemm4 waves split over K; bit 2: the M = 1 decode launch takes the specialised
 * woq_gemv_m1s_kernel, see NAD_GEMV_M1_SPEC; bit 3: ... in its load-ahead order, see NAD_GEMV_AHEAD; from bit 4, where
 * the last main launch is a decode GEMV, the kernel instantiation its launch statement selected, 25 bits from the
 * lowest: family 2 (1 woq_gemv_kernel, 2 woq_gemv_m1_kernel, 3 woq_gemv_m1s_kernel), log2 BITS 2, log2 GPT 2, ASYM 1,
 * AT -- HILO for woq_gemv_kernel -- 2, KSN 3, SPW 3, NST 2, ST + 1 2, BATCH 1, NWT 2, NSC 2 (0, 7, 11, 16), AHEAD 1),
 * launches including pre-passes].  Returns the number of values written or -1. */
#define NAD_KERNEL_GEMV_M1 1   /* woq_gemv_m1_kernel: M = 1 decode */
#define NAD_KERNEL_GEMV 2      /* woq_gemv_kernel: the stripe-stream GEMV, M <= 16 */
#define NAD_KERNEL_SKINNY 3    /* woq_skinny_kernel: decode geometries the stream does not take */
#define NAD_KERNEL_I8 4        /* woq_i8_kernel: int8-compute mode */
#define NAD_KERNEL_GEMM3 5     /* woq_gemm3_kernel: prefill, int4 groups of 128 * 2^j */
#define NAD_KERNEL_GEMM4 6     /* woq_gemm4_kernel: prefill, int4 g32 / g64, int2, int8 */
#define NAD_KERNEL_GEMM2 7     /* woq_gemm2_kernel (NAD_GEMM_KERNEL=2) */
#define NAD_KERNEL_GEMM 8      /* woq_gemm_kernel: register-staged prefill fallback */
#define NAD_KERNEL_GEMM7 9     /* woq_gemm7_kernel: prefill, int4 groups of 128 * 2^j, scale folded (default) */
#define NAD_KERNEL_MID 10      /* woq_mid_kernel: 12 (fp16) / 8 (fp32, bf16) <= M <= 64, int4 / int2 */
#define NAD_KERNEL_Q6K_GEMV 11 /* woq_q6k_gemv_kernel: GGUF Q6_K, M <= 16 (sub-scales in fp32: flags bit 0 clear) */
#define NAD_KERNEL_Q6K_GEMM 12 /* woq_q6k_gemm_kernel: GGUF Q6_K, M > 16 (sc * q folded into fp16: flags bit 0 set) */
#define NAD_KERNEL_Q6K_I8 13   /* woq_q6k_i8_kernel: GGUF Q6_K in mode NAD_COMPUTE_Q8_K, any M (flags bit 0 clear) */
#define NAD_KERNEL_GEMV_ROUTED 14 /* woq_gemv_m1_routed_kernel: expert matmuls routed on the device (nad_plan_moe) */
#define NAD_KERNEL_MOE_COMBINE 15 /* moe_combine_kernel: the weighted sum of the slot results (nad_plan_moe) */
#define NAD_KERNEL_MOE_SORT 16 /* moe_sort_kernel: the problems sorted by expert on the device (nad_plan_moe_grouped) */
#define NAD_KERNEL_CVT_ACT 17  /* nad_cvt_act_kernel: activations -> fp16, K padded to the K tile (nad_plan_moe_grouped) */
#define NAD_KERNEL_GEMM7_GROUPED 18 /* woq_gemm7_grouped_kernel: gemm7 over the sorted rows of routed experts */
#define NAD_KERNEL_MOE_GATHER 19 /* moe_gather_kernel: the slot sum / un-permute over sorted rows (nad_plan_moe_grouped) */
int nad_plan_forward(int bits, int n, int k, int blocksize, int scale_t, int asym, int m, int act_dtype, int64_t* out,
                     int nout);
/* the same dry run for a loaded device weight (its format, act-order, fold range and compute mode included) */
int nad_plan_weight(const void* devstor, int m, int act_dtype, int64_t* out, int nout);
/* Dry runs of nad_device_qkv_forward, for three weight geometries of one format (nq, nk, nv columns; no GPU needed) and
 * for three loaded weights.  out as nad_plan_forward's: the kernel, grid, threads, split-K runs and flags are those of
 * the last main launch, `launches` counts every launch of the call -- a fused gemm7 prefill shows one main launch whose
 * grid covers the column tiles of all three weights, the separate form (NAD_GEMM7_FUSE=0) two launches more. */
int nad_plan_qkv_forward(int bits, int nq, int nk, int nv, int k, int blocksize, int scale_t, int asym, int m,
                         int act_dtype, int64_t* out, int nout);
int nad_plan_qkv(const void* wq, const void* wk, const void* wv, int m, int act_dtype, int64_t* out, int nout);
/* Dry runs of nad_device_ffn_gate_up (SiLU * mul, tmp1 given), for two weight geometries of one format (no GPU needed)
 * and for two weights; out as nad_plan_qkv's.  nad_plan_qkv and nad_plan_gate_up take loaded weights and geometry-only
 * descriptors (nad_weight_plan_only) alike, so fused calls of mixed formats can be asked without a GPU. */
int nad_plan_gate_up_forward(int bits, int n, int k, int blocksize, int scale_t, int asym, int m, int act_dtype,
                             int64_t* out, int nout);
int nad_plan_gate_up(const void* w1, const void* w3, int m, int act_dtype, int64_t* out, int nout);
/* fused Q/K/V (ip_fusion_qkv.cpp:22-93): out_i = X . W_i^T, one launch; W_i share K, blocksize, bits, scale dtype */
int nad_device_qkv_forward(const void* act, int act_dtype, const void* wq, const void* wk, const void* wv, float* oq,
                           float* ok, float* ov, int m, int k, int lda, int ldo_q, int ldo_k, int ldo_v, void* queue);
/* gate/up half of the fused FFN (ip_fusion_ffn.cpp:407-433): tmp2 = act(X.W1^T) * (X.W3^T), tmp1 = act(X.W1^T)
 * (optional for m <= 16).  epi: NAD_EPI_SILU_MUL / NAD_EPI_GELU_MUL. */
int nad_device_ffn_gate_up(const void* act, int act_dtype, const void* w1, const void* w3, float* tmp1, float* tmp2,
                           int m, int fin, int fmid, int lda, int epi, void* queue);
/* fused FFN (ip_fusion_ffn.cpp:407-457): tmp1 = act1(X.W1^T) [optional], tmp2 = tmp1 * (X.W3^T), out = tmp2 . W2^T.
 * epi = NAD_EPI_SILU_MUL or NAD_EPI_GELU_MUL.  tmp1 / tmp2 are scratch: for M > 16 with the pipelined GEMMs they hold
 * the intermediates as fp16 (the down GEMM reads tmp2 as its fp16 operand; NAD_FFN_F32=1 keeps fp32).  The
 * reference-named bestla_fusion_FFN_* entries always return the fp32 intermediates in tmp1 / tmp2. */
int nad_device_ffn_forward(const void* act, int act_dtype, const void* w1, const void* w2, const void* w3, float* tmp1,
                           float* tmp2, float* out, int m, int fin, int fmid, int fout, int lda, int epi, void* queue);
/* tensor-parallel slicing of a packed blob without re-quantization (the reference re-quantizes,
 * model_files.h:1538-1563).  axis 0: split N (TP_1D_ROW, column-parallel) into near-equal chunks of `unit` columns
 * (use the consumer's K group / head size so column shards line up with the next row-parallel weight's K shards);
 * axis 1: split K by whole quantization groups (TP_1D_COLUMN, row-parallel; `unit` ignored).
 * Returns the shard's blob size (dst may be NULL to query). */
size_t nad_blob_split(const void* src, int axis, int rank, int world, int unit, void* dst, size_t dst_capacity);
/* the [begin, end) range of N (axis 0) or K (axis 1) that `rank` owns */
int nad_split_range(const void* src, int axis, int rank, int world, int unit, int* begin, int* end);
/* synthetic device weight of the given geometry (random packed values, scales U[smin,smax], zps) for benchmarks */
int nad_synthetic_weight(void* devstor, void* deviceptr, size_t capacity, int bits, int n, int k, int blocksize,
                         int scale_t, int asym, uint64_t seed, void* queue);
/* device bytes of nad_synthetic_weight's layout */
size_t nad_synthetic_weight_size(int bits, int n, int k, int blocksize, int scale_t, int asym);
/* The host-pointer ABI (bestla_f32f32_forward & co., inner_product.cpp:28-36 called per node at ne_layers.c:7313)
 * keeps one device copy per blob address.  Per call the key check is O(1): the 64-byte header, the blob size and 64
 * dwords sampled at fixed positions; every pack entry of this library (BTLAGemmQuantPackB, BTLAGemmPackB,
 * bestla_packweight_copyattr, nad_blob_split) drops the copy of the buffer it writes, so a rewrite through the pack
 * API is always seen.  The cache is bounded (least recently used first out) by NAD_HOST_CACHE_MB, default 64 GiB. */
void nad_host_cache_clear(void);
/* drop the device copy of one blob.  MUST be called before a blob is freed, or rewritten in place by anything other
 * than this library's pack entries: the per-call key samples the blob, so a partial rewrite (a few groups
 * re-quantized) is not guaranteed to change it, and the forward would use the stale device copy. */
void nad_host_cache_evict(const void* blob);
/* cap on the cached device bytes (0 = the default); returns the previous cap */
size_t nad_host_cache_set_limit(size_t bytes);
/* entries and device bytes currently cached */
int nad_host_cache_stats(size_t* entries, size_t* bytes);
/* the per-call key of a host blob (what the cache compares on every forward); 0 if the blob does not parse */
unsigned long long nad_host_blob_key(const void* blob);
/* ===== int8-compute mode: the reference's comp_int8 arithmetic for weights packed for an integer core (blobs that
 * carry the bf16 reduce).  0 (default): fp16 MFMA on the exact weights.  1: activations quantized to u8 per (row,
 * weight block) as kernel_ref.h:1824-1883, s32 block dot products, the kblock core's fp32 combine
 * (bestla_wrapper.h:768-831, bestla_gemm.h:2983-3050).  Initial value from NAD_COMPUTE_INT8.  Weights without a
 * reduce keep the fp path; a fused call mixing the two kinds fails. */
int nad_set_compute_mode(int mode);
int nad_get_compute_mode(void);
/* per-thread override of the process mode (-1 clears it); thread-safe, takes precedence over nad_set_compute_mode */
int nad_set_thread_compute_mode(int mode);
/* per-weight arithmetic, as the reference selects it per blob core (bestla_gemm.cpp:516-616): -1 follow the
 * thread / process mode, 0 fp, 1 int8 (integer-core blobs and the legacy GGUF block types; other weights -- NFloat
 * weights and GGUF Q6_K among them -- stay fp: the call succeeds and nad_device_get_compute keeps returning 0), or
 * NAD_COMPUTE_Q8_K for a GGUF Q6_K weight: the reference's arithmetic for the type (quantize_fns, ne_layers.c:322-326)
 * -- every activation row quantized to block_q8_K, ggml_vec_dot_q6_K_q8_K's integer dot product per superblock --
 * on woq_q6k_i8_kernel at every M.  Mode 2 on any other weight returns -1 and leaves its mode unchanged; the thread
 * and process modes keep their two values, so a Q6_K weight never follows them into integer arithmetic.  The weight's
 * own mode takes precedence over both; a fused call whose weights resolve to different arithmetic runs each weight in
 * its own. */
#define NAD_COMPUTE_Q8_K 2
int nad_device_set_compute(void* devstor, int mode);
/* the arithmetic a forward of this weight takes now: 0 fp, 1 int8, 2 Q8_K (a Q6_K weight set to it), -1 not a device
 * weight */
int nad_device_get_compute(const void* devstor);
/* kernel::wrapper::QuantizeU8ColBlock::forward (kernel_wrapper.h:571-590) on device pointers: act [m][lda] in
 * act_dtype, q [m][ldq] u8, scales / zps [m][ld_scale] per block, blkreduce (may be NULL) = sum(round(x/s)) * s. */
int nad_quant_u8_colblock(const void* act, int act_dtype, int m, int k, int lda, int blocksize, uint8_t* q, int ldq,
                          float* scales, uint8_t* zps, int ld_scale, float* blkreduce, void* queue);
/* ===== GGUF Q4_0 (neural_speed/core/data_types.h:79-83): a Q4_0 matrix of N rows x K (K % 32 == 0), rows of K/32
 * blocks {fp16 d; u8 qs[16]} as an ne_tensor of type NE_TYPE_Q4_0 holds them, loaded into the same device layout as a
 * BTLA blob (symmetric int4, group 32, fp16 scales); every nad_device_* / bestla_device_* forward then accepts the
 * descriptor.  Compute mode 1 reproduces the reference's Q8_0 x Q4_0 arithmetic (quantize_row_q8_0_reference,
 * ne_vec_dot_q4_0_q8_0). */
size_t nad_q4_0_device_size(int n, int k);
int nad_q4_0_device_load(const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity, void* queue);
/* quantize_row_q8_0 (vectors/cpu/quantize.h:422-445) on device pointers: act [m][lda] -> m rows of K/32 block_q8_0 */
int nad_quant_q8_0(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue);
/* ===== the other legacy GGUF block types the reference matmuls (quantize_fns, neural_speed/core/ne_layers.c:266-318;
 * blocks: core/data_types.h:79-118).  Type codes are the reference's ne_type values.  Q5_0 and Q8_0 load into the
 * symmetric int8 layout, Q5_1 into the int8 layout and Q4_1 into the symmetric int4 layout (the nibble holds q, decoded as q - 8, and the finishing pass adds 8 d with the min); the fp16
 * block minimum of Q4_1 / Q5_1 (w = q d + m) is kept in a region of its own and added by a finishing pass after the
 * forward kernel (two launches per weight, three with the block-sum pre-pass above 16 rows), which also applies the
 * epilogue.  Every nad_device_* / bestla_device_* forward accepts the descriptor.  nad_device_qkv_forward runs the
 * three weights one after another when any carries mins; nad_device_ffn_gate_up / nad_device_ffn_forward run the gate
 * and the up weight as two passes then, and a pair that mixes a min and a non-min weight WORKS as long as the two share
 * the device format the entry requires anyway (bits, group size, scale type; e.g. Q5_1 + Q8_0); such a pair always
 * takes the two-pass path, i.e. it gives up the single dual-weight decode launch of a pair without mins.
 * nad_batch_create refuses a weight with mins (the batched GEMV has no finishing pass).  Compute mode 1
 * reproduces the reference's integer arithmetic: Q8_0 activations for Q5_0 / Q8_0 (ne_vec_dot_q5_0_q8_0,
 * ne_vec_dot_q8_0_q8_0), Q8_1 for Q4_1 / Q5_1 (ne_vec_dot_q4_1_q8_1, ne_vec_dot_q5_1_q8_1); a fused call whose weights
 * need different activation quantizers fails with a recorded error.  NAD_GGUF_Q4_0 through these entries is
 * the load of nad_q4_0_* exactly (one load path serves every type; an error names the entry that was called). */
#define NAD_GGUF_Q4_0 2
#define NAD_GGUF_Q4_1 3
#define NAD_GGUF_Q5_0 6
#define NAD_GGUF_Q5_1 7
#define NAD_GGUF_Q8_0 8
/* bytes of one 32-element block: 18 / 20 / 22 / 24 / 34; 0 and an error naming the type otherwise */
size_t nad_gguf_block_bytes(int type);
/* device bytes of the matrix; 0 and nad_last_error() for an unsupported type or k % 32 != 0 */
size_t nad_gguf_device_size(int type, int n, int k);
int nad_gguf_device_load(int type, const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity,
                         void* queue);
/* ===== GGUF Q6_K (the reference's NE_TYPE_Q6_K; block_q6_K, neural_speed/core/data_types.h:133-138; matmul'd at
 * ne_layers.c:7326 through quantize_fns): a matrix of N rows x K (K % 256 == 0), rows of K/256 superblocks {u8 ql[128];
 * u8 qh[64]; s8 scales[16]; fp16 d} (210 bytes), w = d * scales[e / 16] * q with q in -32..31.  The superblock is 256
 * and the sub-scale group 16, so the type has entries of its own: nad_gguf_block_bytes(14) and nad_gguf_device_size(14,
 * ...) keep returning 0 with an error naming 14.  The device layout holds the file's own 6.5625 bits per weight (6-bit
 * quants as nibble and crumb pieces, int8 sub-scales, fp16 d: nad_q6_k_device_size(n, k) <= ceil(n / 16) * 16 *
 * (k / 256) * 210 + 255), and the weight runs on two kernels of its own: up to 16 rows the decode GEMV, which applies the
 * sub-scales in fp32 (results at the decode tolerance), above that a tile GEMM that folds scales * q into its fp16
 * fragments (the folded-scale tolerance).  nad_weight_info reports bits 6, blocksize 16, scale type f16.  Every
 * nad_device_* / bestla_device_* forward accepts the descriptor with every single-weight epilogue;
 * nad_device_qkv_forward runs the three weights one after another when any is Q6_K; nad_device_ffn_gate_up /
 * nad_device_ffn_forward run gate and up as two passes then, and the partner may be of any format.  Arithmetic is fp
 * by default and under every process / thread mode (nad_device_set_compute(w, 1) leaves it fp);
 * nad_device_set_compute(w, NAD_COMPUTE_Q8_K) switches the weight to the reference's Q8_K integer arithmetic: per
 * (row r, superblock b) isum = sum_g sc[g] * sum_i q[16 g + i] * a[16 g + i] exact in int32 on
 * v_mfma_i32_16x16x64_i8, y = sum_b fp32(fp32(d_w[b]) * d_a[r][b]) * float(isum_b) in fp32 (each wave its superblocks
 * b = wave, wave + 16, ... in ascending order, then the 16 waves in wave order), the rows quantized inside the kernel
 * (one launch at every M, through every entry above).
 * nad_batch_create refuses a Q6_K weight.  nad_device_unpack_fp32 returns (d * sc) * q, bit for bit
 * dequantize_row_q6_K (vectors/cpu/quantize.h:956-999). */
#define NAD_GGUF_Q6_K 14
/* 0 and nad_last_error() unless n > 0 and k is a positive multiple of 256 */
size_t nad_q6_k_device_size(int n, int k);
int nad_q6_k_device_load(const void* blocks, int n, int k, void* devstor, void* deviceptr, size_t capacity, void* queue);
/* ===== ne_get_rows on a device weight (ne_compute_forward_get_rows_q, core/ne_layers.c:8385-8433, 8529-8546: the
 * token embedding of every model graph, models/llama/llama.cpp:189): out[r][0:k] = the dequantized weight row ids[r],
 * i.e. row ids[r] of the [N][K] matrix the weight was quantized from -- the row the forward multiplies the activations
 * by.  Every weight nad_device_load, nad_gguf_device_load, nad_q4_0_device_load, nad_q6_k_device_load and
 * nad_device_quantize produce is taken (int4 / int2 / int8 tile layouts with S1..S8, F4 and F8 codes, every scale type,
 * sym / asym / block mins, both tile orders, Q6_K) except an act-order one, refused by name: "the weight is act-order
 * (desc_act): rows are not gathered from it".
 *   ids   device memory, m entries ids_stride (>= 1) int32s apart: one column of an [m][top_k]-like table is
 *         ids = table + col, ids_stride = top_k.  Read on the device when the kernel runs, never on the host.
 *   out   device memory, [m][ldo] of out_dtype (NAD_ACT_F32 / F16 / BF16), ldo >= k counted in elements.  The rows are
 *         written with 16-byte stores: out must be 16-byte aligned and ldo a multiple of 4 (fp32) / 8 (fp16, bf16)
 *         elements; anything else is refused.  Exactly out[0:m, 0:k] is written.
 * An id outside [0, n) gives a row of +0.0 and reads no weight memory (the index is clamped before any address is
 * formed) -- the rule of an out-of-range expert in the routed entries.
 * fp32 output has the bits of nad_device_unpack_fp32's [kk][ids[r]]: the integer formats float(v - bias - zp) * s, F4
 * the LUT value * s, F8 f8_to_fp32's construction * s, Q4_1 / Q5_1 (q + min_bias) * d then + m each rounded on its own,
 * Q6_K (d * sc) * q; no contraction anywhere.  fp16 / bf16 output is that fp32 value converted once, round to nearest
 * even.
 * One launch; no allocation, no host read of ids, no synchronisation: the call can be captured in a graph and replayed
 * after ids has been rewritten on the device.  m = 0 launches nothing.  Returns 0, or -1 and nad_last_error(). */
int nad_device_get_rows(const void* devstor, const int32_t* ids, int ids_stride, int m, void* out, int out_dtype,
                        int ldo, void* queue);
/* Dry run of nad_device_get_rows (no launch, no GPU needed; a geometry-only descriptor qualifies): out as
 * nad_plan_weight's -- [NAD_KERNEL_GET_ROWS, grid, threads per workgroup, 1, 0, launches]; a unit of work is (row, 16 K
 * tiles) -- Q6_K: (row, 4 superblocks) -- and a workgroup takes four.  Returns the number of values written or -1. */
#define NAD_KERNEL_GET_ROWS 20 /* woq_get_rows_kernel / woq_get_rows_q6k_kernel: ne_get_rows on a device weight */
#define NAD_KERNEL_GEMV_ROUTED_GENERAL 21 /* woq_gemv_routed_kernel: routed expert matmuls of a general bank's int4 g32 /
                                             int8 weights on the stripe stream (nad_plan_moe) */
#define NAD_KERNEL_Q6K_GEMV_ROUTED 22 /* woq_q6k_gemv_routed_kernel: routed expert matmuls of a bank of GGUF Q6_K experts,
                                        one fp32 row per problem (nad_plan_moe) */
#define NAD_KERNEL_Q6K_GEMM_GROUPED 23 /* woq_q6k_gemm_grouped_kernel: the Q6_K GEMM over the sorted rows of routed
                                          experts, 128-row tiles (nad_plan_moe_grouped) */
int nad_plan_get_rows(const void* devstor, int m, int out_dtype, int64_t* out, int nout);
/* A geometry-only weight descriptor for the dry runs, no GPU needed: bits 2 / 4 / 8 (blocksize <= 0 = per-channel,
 * scale_t NAD_SCALE_*, act_order != 0: a desc_act weight) or 6 (Q6_K, k % 256 == 0; the other arguments are ignored).
 * It holds no weights: nad_plan_get_rows and the argument checks of nad_device_get_rows take it, every entry that
 * would launch on it refuses it by name. */
int nad_weight_plan_only(int bits, int n, int k, int blocksize, int scale_t, int asym, int act_order, void* devstor);
/* quantize_row_q8_1_reference (vectors/cpu/quantize.h:546-579) on device pointers: act [m][lda] -> m rows of K/32
 * blocks {float d; float s; int8 qs[32]} */
int nad_quant_q8_1(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue);
/* quantize_row_q8_K_reference (vectors/cpu/quantize.h:1020-1055) on device pointers: act [m][lda] in act_dtype
 * -> m rows of k/256 blocks {float d; int8 qs[256]; int16 bsums[16]} (292 bytes); k % 256 == 0.  Bit for bit the
 * reference for finite inputs whose per-superblock largest magnitude is zero or an fp32 normal; an all-zero superblock
 * gets d = 0, codes 0 and bsums 0 (the reference leaves bsums unwritten there).  Bad arguments: -1 before anything on
 * the device is touched. */
int nad_quant_q8_k(const void* act, int act_dtype, int m, int k, int lda, void* blocks, void* queue);
/* host convenience: (re)pack one blob into fp32 dequantized [K][N] from the device tile layout (round-trip check) */
int nad_device_unpack_fp32(const void* devstor, float* host_out, void* queue);

/* ===== batched independent decode problems: BTLAGemmBatchDriver (bestla_gemm.cpp:508-624) for device tensors.  n
 * problems y_i = x_i W_i (M = 1, fp32 x_i [K] 16-B aligned, fp32 y_i [N]) whose weights share N, K and format (int4 /
 * int2, no act-order, fp arithmetic, a geometry the M = 1 GEMV takes) run as ONE launch: workgroups are dealt out
 * problem by problem, each streaming its problem's share of the stripes.  The pointers are bound at creation (a device
 * problem table): keep the tensors alive and reuse them across runs; run is asynchronous on queue and graph-capturable.
 * create returns NULL with nad_last_error() set when the problems do not qualify. */
typedef struct nad_batch_problem {
  const void* weight; /* a loaded device weight (bestla_device_load_storage / nad_device_load) */
  const float* act;   /* [K] */
  float* out;         /* [N] */
} nad_batch_problem;
void* nad_batch_create(const nad_batch_problem* problems, int n);
int nad_batch_run(void* batch, void* queue);
/* dry run of nad_batch_run: out as nad_plan_forward's (nothing is launched) */
int nad_plan_batch(void* batch, int64_t* out, int nout);
/* the same dry run for n problems on one weight, loaded or geometry-only (nad_weight_plan_only): no GPU needed */
int nad_plan_batch_only(const void* devstor, int n, int64_t* out, int nout);
void nad_batch_destroy(void* batch);

/* ===== routed expert matmuls: ne_mul_mat_id / ne_mul_id_ffn_silu (neural_speed/core/ne_layers.c:2384-2462, 7783-7916,
 * 8053-8075), the FFN of every layer of the Llama graph once n_expert > 0 (models/llama/llama.cpp:620-688).  The
 * expert of a row is an int32 in DEVICE memory, read inside the launch: nothing here copies ids to the host,
 * synchronises, allocates or frees, so a routed layer is graph-capturable and a replay follows whatever the router wrote
 * since.  Activations and outputs are fp32.
 *
 * Expert bank: n_expert (1..256) loaded device weights of one shape and format, under nad_batch_create's conditions
 * -- int4 / int2 tile layouts, no act-order, fp arithmetic, no block mins, no Q6_K, a geometry the M = 1 GEMV takes;
 * create returns NULL with nad_last_error() naming the offending expert otherwise.  The bank owns one device table of
 * 64-byte entries (the only allocation of these entries); keep the weights alive while it is. */
void* nad_expert_bank_create(const void* const* weights, int n_expert);
/* a geometry-only bank for nad_plan_moe, with the same checks and no GPU needed: geom holds n_expert rows of
 * [bits (2, 4, 8; 6 = GGUF Q6_K), n, k, blocksize (<= 0: per-channel), NAD_SCALE_*, asym].  It holds no weights: the
 * launching entries below refuse it (-1). */
void* nad_expert_bank_plan_only(const int32_t* geom, int n_expert);
/* The same two entries with flags.  flags = 0: exactly the entries above ("a bank that exists runs on the M = 1
 * stream").  NAD_BANK_GENERAL: the bank also takes the weights that the stripe-stream GEMV (woq_gemv_kernel, hi / lo
 * fp16 rows) runs at M = 1 with fp32 rows and the M = 1 stream does not:
 *   int4 groups of 32, symmetric (the reference's default quantization; GGUF Q4_0)
 *   int8 groups of 32 or 64 * 2^j, per-channel included, symmetric or asymmetric (S8, S5..S7; GGUF Q8_0, Q5_0)
 * with any scale type.  Such a bank is served by woq_gemv_routed_kernel (route kind 1) under the same contract: every
 * routed row bit-identical to the expert's own M = 1 forward, ids read on the device, one launch per matmul.  A bank
 * whose format the M = 1 stream takes is the bank the entries above make (route kind 0), whichever entry made it.
 * A bank whose experts are ALL GGUF Q6_K of one shape is route kind 2 (bits 6, group 16): its table entries hold the
 * three quant pieces (tiles), d (scales) and the sub-scales (zps), and woq_q6k_gemv_routed_kernel serves it -- the
 * dense Q6_K GEMV's body, a problem being one fp32 row, max(1, min(stripes, CUs / problems)) workgroups per problem,
 * every routed row bit-identical to the expert's own M = 1 forward.  There an id outside [0, n_expert) reads neither
 * weights nor activations: the row is +0.0 whatever the activations hold.  K up to 32768 (the row's hi and lo fp16
 * images beside 32 KiB of partial sums in 160 KiB of LDS); a longer K is refused by name at the call.
 * Still refused, by name: block mins (Q4_1 / Q5_1), a Q6_K expert beside experts of another format, a Q6_K weight in
 * mode NAD_COMPUTE_Q8_K (integer arithmetic), NFloat codes, act-order, integer-compute weights, and int4 groups of 32
 * with zero points (the skinny kernel's).  The gate / up pair and the down bank of one FFN may be of different kinds
 * (Q4_0 or Q6_K gate / up with an int4 g128 down, int4 g128 gate / up with a Q6_K down). */
#define NAD_BANK_GENERAL 1u
void* nad_expert_bank_create_ex(const void* const* weights, int n_expert, unsigned flags);
void* nad_expert_bank_plan_only_ex(const int32_t* geom, int n_expert, unsigned flags);
void nad_expert_bank_destroy(void* bank);
/* [n_expert, bits, n, k, blocksize, scale_t, asym, holds weights, route kind (0 the M = 1 stream, 1 the stripe stream, 2 the
 * Q6_K GEMV)];
 * writes min(nout, 9) values, returns the count or -1 */
int nad_expert_bank_info(const void* bank, int64_t* out, int nout);
/* ne_mul_mat_id: out[r][0:n] = act[r][0:k] . W[ids[r * ids_ld + slot]]^T for r < m, ONE launch
 * (woq_gemv_m1_routed_kernel: workgroups dealt out row by row, each row exactly the arithmetic of its expert's own M = 1
 * forward -- bit-identical to it).  ids is device memory.  An id outside [0, n_expert) is defined: no weight memory is
 * touched, the row's activations meet all-zero weights and scales, and the row is written as zeros -- for activations
 * that are finite and whose fp16 hi part is finite (|x| below 65520); an inf, NaN or larger value gives NaN (0 * inf).  Writes exactly out[0:m, 0:n] whatever out held; reads act only inside
 * [0:m, 0:k].  Rows need lda % 4 == 0 and a 16-byte aligned base: otherwise -1 before anything is launched.
 * Every row streams its expert's whole weight, also where several rows chose the same expert: right for decode-size m,
 * correct but wasteful at prefill sizes: there nad_device_mul_mat_id_grouped / nad_device_moe_ffn_grouped (below) read
 * every expert's weight once.  The caller chooses; nothing switches between the two forms by itself.  Measured on
 * Mixtral-8x7B shapes (8 experts, top-2, int4 g128; profiles/moe_grouped_times.txt): the grouped
 * FFN has a floor of about 220 us per layer call, so this form is ahead at M = 4 (128 us) and behind from M = 16 on
 * (432 against 222 us; M = 2048: 58.5 against 1.85 ms). */
int nad_device_mul_mat_id(const void* bank, const float* act, const int32_t* ids, int ids_ld, int slot, float* out,
                          int m, int lda, int ldo, void* queue);
/* The whole routed FFN (llama.cpp:641-679) in three launches.  Problem p = r * top_k + i uses expert e = ids[r * ids_ld
 * + i]:
 *   1. t[p] = act1(x_r . G_e^T) * (x_r . U_e^T)   the fused pair epilogue of the M = 1 GEMV, epi = NAD_EPI_SILU_MUL or
 *                                                  NAD_EPI_GELU_MUL; workspace rows [p][fmid] at offset 0
 *   2. y[p] = t[p] . D_e^T                          workspace rows [p][fout] at offset round256(m * top_k * fmid * 4)
 *   3. out[r][n] = ((w[r][0] * y[r * top_k][n]) + w[r][1] * y[r * top_k + 1][n]) + ...   with w[r][i] = wts[r * wts_ld
 *      + i]: fp32, every product and sum rounded on its own, in slot order (ne_mul then ne_add) -- numpy float32
 *      reproduces it bit for bit.
 * t[p] and y[p] are bit-identical to nad_device_ffn_gate_up / nad_device_forward of that expert on that row alone.  A
 * slot whose id is outside [0, n_expert) has t = y = 0 and contributes w * 0 (finite activations, as above).  The gate
 * and up banks must agree in K, N, bits, group size, scale type and symmetry; the down bank may differ in format (the
 * int2 policy keeps it int4, llama_utils.cpp:269-287).  workspace: nad_moe_workspace_size(m, top_k, fmid, fout) = round256(m * top_k * fmid * 4) +
 * round256(m * top_k * fout * 4) bytes (round256: up to a multiple of 256), 16-byte aligned.  The window contract of
 * nad_device_mul_mat_id holds for act and out.
 * Q6_K gate / up banks (route kind 2) run step 1 as the dense Q6_K FFN does, in two launches on the same rows of t --
 * t[p] = act1(x_r . G_e^T), then t[p] = t[p] * (x_r . U_e^T) in place, the lane that reads an element writing it -- so
 * the call is four launches; the workspace and the bit-identity of t[p] and y[p] are the same.  Each launch is served
 * by its own bank's kernel, whatever the kinds of the other banks. */
size_t nad_moe_workspace_size(int m, int top_k, int fmid, int fout);
int nad_device_moe_ffn(const void* gate_bank, const void* up_bank, const void* down_bank, const float* act,
                       const int32_t* ids, int ids_ld, const float* wts, int wts_ld, int top_k, int epi,
                       void* workspace, float* out, int m, int lda, int ldo, void* queue);
/* The router (llama.cpp:624-638), one wave per row, n_expert <= 64, 1 <= top_k <= n_expert, all in fp32:
 *   p = softmax(logits[r]) with the row maximum subtracted: expf(x - max) / sum, the sum a butterfly over the lanes
 *   ids[r][0:top_k] = the indices of the top_k largest p in descending order, a tie going to the lower index
 *   wts[r][i] = p[ids[r][i]] / (p[ids[r][0]] + p[ids[r][1]] + ...), the sum added in slot order
 * It is defined by this arithmetic and is NOT the reference's ne_soft_max, whose expf reads an fp16 table
 * (ne_layers.c): weights agree with it to fp16 table precision only, and near-ties may order differently. */
int nad_moe_route(const float* logits, int ld, int m, int n_expert, int top_k, int32_t* ids, int ids_ld, float* wts,
                  int wts_ld, void* queue);
/* The router from the hidden state: logits = the ffn_gate_inp matmul (llama.cpp:631, grok.cpp:292) of an UNQUANTIZED
 * gate, then nad_moe_route's arithmetic on them, in ONE launch (moe_gate_route_kernel: one workgroup of 1024 threads
 * per row, no workspace, no atomics, nothing between workgroups).  Nothing is copied to the host, synchronised or
 * allocated: graph-capturable, and a replay follows act and gate as they are rewritten on the device.
 *   act    device memory, fp32 [m][lda]
 *   gate   device memory, [n_expert][ldw] of gate_dtype: NAD_ACT_F32, NAD_ACT_F16 or NAD_ACT_BF16 (what
 *          convert_quantized_mixtral.py and GGUF files keep ffn_gate_inp.weight as)
 * Arithmetic, part of the ABI like nad_moe_route's.  For row r and expert e let x = act[r] and w = gate[e], an fp16 or
 * bf16 w widened exactly to fp32.  Every product and every sum below is an fp32 operation rounded on its own (no fused
 * multiply-add):
 *   slots   1024 slots t, each starting at +0.0f.  For pass i = 0, 1, ... and j = 0..3 in that order slot t adds
 *           x[k] * w[k] with k = 4 (t + 1024 i) + j; elements with k >= K are skipped (the same as adding +0.0f: a sum
 *           that starts at +0.0f never becomes -0.0f).
 *   waves   the 64 slots of wave t >> 6 are summed by the xor butterfly s = s + shfl_xor(s, o), o = 32, 16, ..., 1
 *           (addition commutes, so every lane ends with the same value).
 *   row     the 16 waves' sums are added in wave order: logit = ((s0 + s1) + s2) + ... + s15.
 *   route   ids and wts are nad_moe_route's function of these logits (the same device code computes them).
 * The result for a row depends on that row, the gate and K alone: not on m, the row's index, n_expert, the grid, or the
 * gate's storage type (an fp16 gate gives the bits of its fp32 widening).  A token is routed the same alone and inside
 * a prompt.  numpy float32 reproduces the logits bit for bit (tests/gate_model.py); against the exact dot product
 * they lie within depth * 2^-24 * sum |x_k w_k|, depth = 4 * passes + 6 + 15 + 1, passes = ceil(K / 4096).
 * Non-finite logits are as undefined as in nad_moe_route.
 * Windows: writes exactly ids[0:m, 0:top_k] and wts[0:m, 0:top_k], and logits[0:m, 0:n_expert] when logits is not
 * NULL; reads act and gate only inside [.., 0:k].
 * Refused with -1 before any launch, nad_last_error() naming the argument: a null act, gate, ids or wts; m < 0; k < 4
 * or k % 4 != 0; n_expert outside 1..64; top_k outside 1..n_expert; an unknown gate_dtype; lda or ldw below k or not a
 * multiple of 4; ids_ld or wts_ld below top_k; logits_ld below n_expert when logits is given; act or gate not 16-byte
 * aligned.  m == 0 returns 0 and launches nothing.
 * Not for a gate that the reference's quantizer turned into a BTLA blob (nad_device_forward + nad_moe_route serve
 * that), and not the reference's ne_soft_max (see nad_moe_route). */
#define NAD_KERNEL_MOE_GATE_ROUTE 24 /* moe_gate_route_kernel: the gate matmul and the router of one row per workgroup */
int nad_moe_gate_route(const float* act, int lda, const void* gate, int gate_dtype, int ldw, int m, int k, int n_expert,
                       int top_k, int32_t* ids, int ids_ld, float* wts, int wts_ld, float* logits, int logits_ld,
                       void* queue);
/* Dry run of nad_moe_gate_route (no launch, no GPU needed), m >= 1: [NAD_KERNEL_MOE_GATE_ROUTE, grid = m, 1024, dynamic
 * LDS bytes = 16 * n_expert * 4, the launch count 1].  Writes min(nout, 5), returns the number written or -1 (the
 * entry's own refusals, by the same texts). */
int nad_plan_moe_gate_route(int m, int k, int n_expert, int top_k, int gate_dtype, int64_t* out, int nout);
/* Dry run of nad_device_moe_ffn (no launch, no GPU needed; geometry-only banks qualify): per launch [kernel
 * NAD_KERNEL_*, grid, threads per workgroup, dynamic LDS bytes] -- 1 gate + up, 2 down (each NAD_KERNEL_GEMV_ROUTED, or
 * NAD_KERNEL_GEMV_ROUTED_GENERAL for a bank of route kind 1, NAD_KERNEL_Q6K_GEMV_ROUTED for kind 2; grid = m * top_k *
 * workgroups per problem), 3 combine -- then the launch count: 13 values.  Q6_K gate / up banks: 1 gate, 2 up, 3 down,
 * 4 combine, then the count: 17 values.  The last value written of a full record is the launch count.  Writes
 * min(nout, that), returns the number written or -1. */
int nad_plan_moe(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k, int64_t* out,
                 int nout);

/* ===== the same, sorted and grouped: for prefill-size m.  The problems p = r * top_k + i (expert e_p = ids[r * ids_ld +
 * i], valid when 0 <= e_p < n_expert) are sorted by (e_p, p) ON THE DEVICE, and every expert's rows run through gemm7's
 * tile kernel (woq_gemm7_grouped_kernel: MFMA, the expert's weight read once per 32 .. 256 rows instead of once per
 * row).  As above nothing copies ids to the host, synchronises, allocates or frees: graph-capturable, and a replay
 * follows the ids it finds.  The sort is a function of ids alone (a stable counting sort, no atomics).
 *
 * A bank is taken when every expert's format is one gemm7 has (recorded at bank creation): int4 groups of 64 or
 * 128 * 2^j, int2 groups of 64 * 2^j, and for a bank of route kind 1 (NAD_BANK_GENERAL) int4 groups of 32 and int8
 * groups of 32 or 64 * 2^j, sym or asym, any
 * scale type, every q * s inside the fp16 range (geometry-only banks count as such) -- and every bank of route kind 2
 * (GGUF Q6_K), which woq_q6k_gemm_grouped_kernel serves: the dense Q6_K GEMM's body (128 x 128 tiles, fp16(sc * q)
 * fragments, d applied in fp32 per superblock) with the tile -> (expert, rows) map of the sort and the weight pointers
 * of the bank's table.  As soon as one bank of a call is Q6_K the tile height of the whole call is 128 (NAD_GEMM7_BM
 * does not apply; gemm7's grouped kernel serves the other banks at 128).  The FFN also needs fmid to be a whole number
 * of the down bank's K tiles (128 int4, 256 int2, 64 int8, 256 Q6_K).  Anything else: -1 before any launch, nad_last_error() naming the bank and the reason -- never the
 * row-routed path in its place.
 *
 * Arithmetic: the activations are rounded to fp16 and q * s is rounded once to fp16, as in every gemm7 forward; an
 * output element's MFMA sequence does not depend on the other rows of its tile, so y for (x_r, e) is bit-identical
 * whatever else is in the batch, whatever the tile height, and to nad_device_forward of expert e on fp16 rows where
 * that runs gemm7 without split K (a Q6_K bank: where that runs woq_q6k_gemm_kernel, M > 16).  The FFN keeps act1(gate) and act1(gate) * up as fp16 (the dense prefill FFN's
 * intermediates) and y in fp32.
 *
 * Workspace (16-byte aligned, nad_moe_grouped_workspace_size bytes; np = m * top_k; every part starts at the next
 * multiple of 256 bytes after the one before):
 *   offs  int32 [n_expert + 1]   expert e owns sorted rows offs[e] .. offs[e + 1] - 1; offs[n_expert] = valid problems
 *   perm  int32 [np]             the valid problems by (e_p, p); -1 from offs[n_expert] on
 *   src   int32 [np]             perm[q] / top_k; 0 from offs[n_expert] on
 *   inv   int32 [np]             the sorted position of p, -1 for an invalid id
 *   tiles int32 count, 12 bytes unused, then int32 [np / 32 + min(n_expert, np)][4] = (e, q0, q1, 0): per expert
 *         ceil(count_e / BM) tiles of at most BM sorted rows, BM the call's tile height
 *   x16   fp16 [m][kp]           the activations, kp = K rounded up to the gate bank's K tile (Q6_K: kp = K)
 *   t16   fp16 [np][fmid]        FFN only: act1(x . G_e^T) by sorted row
 *   u16   fp16 [np][fmid]        FFN only: t16 * (x . U_e^T)
 *   y     fp32 [np][fout]        the sorted result rows (fout: the down bank's N; one matmul: the bank's N)
 * up_bank = down_bank = NULL sizes the one-matmul form (top_k = 1).  Every word a launch reads is rewritten by the
 * call; rows of t16 / u16 / y from offs[n_expert] on are not written. */
size_t nad_moe_grouped_workspace_size(const void* gate_bank, const void* up_bank, const void* down_bank, int m,
                                      int top_k);
/* nad_device_moe_ffn's arguments and result contract, in six launches: sort; x -> fp16; gate (act1 -> t16); up (t16 *
 * product -> u16); down (-> y); out[r][n] = ((w[r][0] * y[inv[r * top_k]][n]) + w[r][1] * y[inv[r * top_k + 1]][n]) +
 * ... with nad_device_moe_ffn's combine arithmetic, an invalid slot contributing w * 0.0f.  Writes exactly
 * out[0:m, 0:fout]; reads act only inside [0:m, 0:fin]; rows need lda % 4 == 0 and a 16-byte aligned base. */
int nad_device_moe_ffn_grouped(const void* gate_bank, const void* up_bank, const void* down_bank, const float* act,
                               const int32_t* ids, int ids_ld, const float* wts, int wts_ld, int top_k, int epi,
                               void* workspace, float* out, int m, int lda, int ldo, void* queue);
/* ne_mul_mat_id grouped: sort (by ids[r * ids_ld + slot]); x -> fp16; one grouped GEMM into y; out[r] = y[inv[r]], or a
 * zero row for an id outside [0, n_expert).  Same window contract. */
int nad_device_mul_mat_id_grouped(const void* bank, const float* act, const int32_t* ids, int ids_ld, int slot,
                                  void* workspace, float* out, int m, int lda, int ldo, void* queue);
/* Dry run of the grouped entries (no launch, no GPU needed; geometry-only banks qualify): per launch [kernel
 * NAD_KERNEL_*, grid, threads per workgroup, dynamic LDS bytes], then the tile height BM (gemm7's choice for m * top_k /
 * n_expert rows, or NAD_GEMM7_BM; 128 with a Q6_K bank in the call, whose GEMMs are NAD_KERNEL_Q6K_GEMM_GROUPED with 512
 * threads and static LDS, recorded as 0), the tile bound floor(m * top_k / BM) + min(n_expert, m * top_k) -- a grouped GEMM's
 * grid is that bound times its column tiles of 128 -- and the launch count.  FFN: 6 launches, 27 values; up_bank =
 * down_bank = NULL (top_k = 1): 4 launches, 19 values.  Writes min(nout, that), returns the number written or -1. */
int nad_plan_moe_grouped(const void* gate_bank, const void* up_bank, const void* down_bank, int m, int top_k,
                         int64_t* out, int nout);

#ifdef __cplusplus
}
#endif
#endif /* NEURAL_AMD_H */
