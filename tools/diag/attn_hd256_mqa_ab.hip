// attn_hd256_mqa_ab.hip -- A/B arm of attention variant 4 (llama_attn_hd256.hip): one head per workgroup (the product) vs
// two heads of one KV head per workgroup sharing each staged K/V tile. Built into a small shared library next to the
// product one by tools/diag/attn_hd256_mqa_ab.py, which times both forms in one process and checks they give the same bits.
#include "../../llamarec_amd/csrc/llama_attn_hd256.hip"

extern "C" int diag_attn_hd256(const unsigned short* qkv, unsigned short* out, const int32_t* cu, const int32_t* cu_host, int B,
                               int n_tok, int nh, int nkv, int heads_per_wg, void* stream) {
  if (heads_per_wg == 2) return launch_hd256<2>(qkv, out, cu, cu_host, B, n_tok, nh, nkv, 256, (hipStream_t)stream);
  return launch_hd256<1>(qkv, out, cu, cu_host, B, n_tok, nh, nkv, 256, (hipStream_t)stream);
}
