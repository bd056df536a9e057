// status strings / version of libvilco_hip.so
#include <string.h>
#include "common.h"

extern "C" const char* vilco_status_str(int status) {
  switch (status) {
    case VILCO_OK: return "ok";
    case VILCO_ERR_BADARG: return "vilco_hip: bad argument (null pointer, negative size or misaligned operand)";
    case VILCO_ERR_UNSUPPORTED: return "vilco_hip: shape not supported by the gfx950 kernels";
    case VILCO_ERR_LAUNCH: return "vilco_hip: kernel launch failed";
    case VILCO_ERR_WORKSPACE: return "vilco_hip: workspace too small";
    default: return "vilco_hip: unknown status";
  }
}

extern "C" const char* vilco_version(void) { return "vilco_hip 0.1 gfx950"; }

extern "C" size_t vilco_abi_sizeof(const char* struct_name) {
#define ABI_SIZE(T) if (struct_name && !strcmp(struct_name, #T)) return sizeof(T);
  ABI_SIZE(vilco_gemm_desc) ABI_SIZE(vilco_pack_item) ABI_SIZE(vilco_attn_amax_in) ABI_SIZE(vilco_loss_desc)
  ABI_SIZE(vilco_ln_fwd_desc) ABI_SIZE(vilco_ln_bwd_desc) ABI_SIZE(vilco_attn_desc) ABI_SIZE(vilco_scale_add_bwd_desc)
  ABI_SIZE(vilco_act_bwd_desc) ABI_SIZE(vilco_optim_desc) ABI_SIZE(vilco_distill_desc) ABI_SIZE(vilco_bic_correct_desc)
  ABI_SIZE(vilco_prompt_desc) ABI_SIZE(vilco_si_desc) ABI_SIZE(vilco_chunk_table) ABI_SIZE(vilco_der_desc)
  ABI_SIZE(vilco_coda_desc) ABI_SIZE(vilco_rwalk_step_desc) ABI_SIZE(vilco_rwalk_desc) ABI_SIZE(vilco_pod_desc)
  ABI_SIZE(vilco_erd_desc) ABI_SIZE(vilco_erd_select_desc)
#undef ABI_SIZE
  return 0;
}

// The device status word: kernels that validate device-resident arguments OR a bit into it (an integer atomic) instead of
// faulting or making the host read; vilco_status_word_take reads and clears it.
__device__ int32_t vilco_status_word_storage[16];      // word 0; its own 64-byte line

int32_t* vilco_status_word_dev() {
  static int32_t* p = [] {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(vilco_status_word_storage)) != hipSuccess) q = nullptr;
    return reinterpret_cast<int32_t*>(q);
  }();
  return p;
}

// current value, then cleared (synchronises the device: tests / end-of-epoch checks only)
extern "C" int vilco_status_word_take(int32_t* out) {
  if (!out) return VILCO_ERR_BADARG;
  if (hipDeviceSynchronize() != hipSuccess) return VILCO_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vilco_status_word_storage), sizeof(int32_t)) != hipSuccess) return VILCO_ERR_LAUNCH;
  const int32_t zero = 0;
  return hipMemcpyToSymbol(HIP_SYMBOL(vilco_status_word_storage), &zero, sizeof(int32_t)) == hipSuccess ? VILCO_OK : VILCO_ERR_LAUNCH;
}
