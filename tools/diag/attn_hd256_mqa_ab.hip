// attn_hd256_mqa_ab.hip -- A/B arm of attention variant 4 (llama_attn_hd256.hip): one head per workgroup (the product) vs
// two heads of one KV head per workgroup sharing each staged K/V tile. Built into a small shared library next to the
// product one by tools/diag/attn_hd256_mqa_ab.py, which times both forms in one process and checks they give the same bits.
#include "../../llamarec_amd/csrc/llama_attn_hd256.hip"

extern "C" int diag_attn_hd256(const unsigned short* qkv, unsigned short* out, const int32_t* cu, const int32_t* cu_host, int B,
                               int n_tok, int nh, int nkv, int heads_per_wg, void* stream) {
  LrAttnArgs a = {};
  a.qkv = qkv, a.out = out, a.cu = cu, a.cu_host = cu_host;
  a.S = B, a.n_tok = n_tok, a.nh = nh, a.nkv = nkv, a.hd = 256;
  return heads_per_wg == 2 ? launch_hd256<2>(a, (hipStream_t)stream) : launch_hd256<1>(a, (hipStream_t)stream);
}
