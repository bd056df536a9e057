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
#undef ABI_SIZE
  return 0;
}
