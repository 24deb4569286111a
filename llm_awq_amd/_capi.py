"""ctypes view of the C ABI (include/awq_cdna4.h) -- used by the host-side format tools, by
`llm_awq_amd.ops` and by the parity tests (which must call through the C ABI).

There is NO fallback: if libawq_cdna4.so is missing this module raises at first use.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (AWQ_CDNA4_LIB: another build of the same library, e.g. an AWQ_PROBES=1 build kept beside the product one for timing experiments)
LIB_PATH = os.environ.get("AWQ_CDNA4_LIB") or os.path.join(_HERE, "lib", "libawq_cdna4.so")

AWQ_F16, AWQ_BF16 = 0, 1
AWQ_F32 = 2  # router logits of awq_moe_route, logits of awq_sample_logits and the fp32 output of awq_lm_head only
AWQ_SAMPLE_APPEND, AWQ_SAMPLE_ADVANCE = 1, 2  # flags of awq_sample_logits
AWQ_ERR_WORKSPACE = -7  # include/awq_cdna4.h
_lib = None

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
SIGNATURES = {
    "awq_abi_version": (_i, []),
    "awq_status_string": (ctypes.c_char_p, [_i]),
    "awq_last_hip_error": (ctypes.c_char_p, []),
    "awq_w4a16_gemv": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_gemm_workspace_bytes": (_sz, [_i, _i, _i]),
    "awq_w4a16_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_w4a16_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_unpack_v2": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_dequant_v2": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_pack_v2": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_repack_v1_to_v2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_repack_v2_to_cdna4": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_repack_cdna4_to_v2": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_unpack_cdna4": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_dequant_cdna4": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_pack_sz_cdna4": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "awq_pack_szh_cdna4": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "awq_w4a16_decode_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_gemv_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_mlp_gate_up_cdna4": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_mlp_gate_up_forward_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes": (_sz, [_i, _i, _i]),
    "awq_w4a16_mlp_gate_up_forward_cdna4_ws": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_w4a16_rmsnorm_forward_cdna4": (_i, [_vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_rmsnorm": (_i, [_vp, _vp, ctypes.c_float, _vp, _i, _i, _i, _vp]),
    "awq_w4a16_forward_cdna4_workspace_bytes": (_sz, [_i, _i, _i]),
    "awq_midm_init": (_i, []),
    "awq_w4a16_gemm_cdna4_plan": (_i, [_i, _i, _i, _vp, _vp]),
    "awq_w4a16_gemm_cdna4_pair_plan": (_i, [_i, _i, _i]),
    "awq_w4a16_gemm_cdna4_pair_lost": (_i, [_vp]),
    "awq_w4a16_gemm_cdna4_narrow_kernel": (_i, [_i, _i, _i, _i, _i, _i]),
    "awq_w4a16_decode_cdna4_plan": (_i, [_i, _i, _i, _i, _vp]),
    "awq_w4a16_decode_cdna4_plan_detail": (_i, [_i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_linear_route_cdna4": (_i, [_i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_gemm_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_w4a16_forward_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_w4a16_forward_cdna4_szh": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_w4a16_moe_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_moe_forward_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_moe_forward_cdna4_szh": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_silu_mul": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "awq_w4a16_moe_mlp_gate_up_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_w4a16_moe_mlp_gate_up_cdna4_szh": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_moe_route": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "awq_moe_gather": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_moe_combine": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_sample_logits": (_i, [_vp, _i, _i, _i] + [_vp] * 7 + [_i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp]),
    "awq_spec_draft_ngram": (_i, [_vp] * 6 + [_i] * 7 + [_vp]),
    "awq_spec_pack": (_i, [_vp] * 6 + [_i] * 3 + [_vp]),
    "awq_spec_verify": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i] + [_vp] * 6 + [_i, _vp, _vp]),
    "awq_spec_accept": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "awq_lm_head": (_i,[_vp, ctypes.c_long, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_lm_head_plan": (_i, [_i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "awq_embed_tokens": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_lm_head_logprobs": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_float] + [_vp] * 7 + [_i] * 5 + [_vp, _sz, _i, _vp]),
    "awq_lm_head_logprobs_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "awq_lm_head_logprobs_plan": (_i, [_i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "awq_token_logprobs": (_i, [_vp, _i, ctypes.c_long, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    # final-logit soft-capping: softcap in front of max_blocks / behind round_logits, and logits capped in place
    "awq_lm_head_softcap": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_float, _i, _vp]),
    "awq_lm_head_logprobs_softcap": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_float] + [_vp] * 7 + [_i] * 5 + [ctypes.c_float, _vp, _sz, _i, _vp]),
    "awq_logit_softcap": (_i, [_vp, _i, ctypes.c_long, _vp, _i, _i, ctypes.c_float, _vp]),
    "awq_lora_plan": (_i, [_i, _i, _i, ctypes.POINTER(ctypes.c_int)]),
    "awq_lora_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "awq_lora_shrink": (_i, [_vp, ctypes.c_long, _vp, _vp, _vp, _vp, _sz] + [_i] * 8 + [_vp]),
    "awq_lora_expand": (_i, [_vp, _sz, _vp, _vp, _vp, _vp, _vp] + [_i] * 7 + [ctypes.POINTER(ctypes.c_int), _i, _i, _vp]),
    "awq_lora_expand_gate_up": (_i, [_vp, _sz] + [_vp] * 6 + [_i] * 8 + [_vp]),
    "awq_quantize_group": (_i, [_vp, ctypes.c_long] + [_vp] * 7 + [_i] * 6 + [_vp]),
    "awq_quantize_group_host": (_i, [_vp, ctypes.c_long] + [_vp] * 7 + [_i] * 5),
    "awq_clip_search": (_i, [_vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _vp] + [_i] * 8 + [_vp]),
    "awq_pack_w3": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_unpack_w3": (_i, [_vp, _vp, _i, _i, _vp]),
    "awq_dequant_w3": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_w3a16_forward_workspace_bytes": (_sz, [_i, _i, _i]),
    "awq_w3a16_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_oneshot_buffer_bytes": (_sz, [_i, _i]),
    "awq_oneshot_alloc": (_i, [ctypes.POINTER(_vp), _i, _i]),
    "awq_oneshot_free": (_i, [_vp]),
    "awq_oneshot_ipc_export": (_i, [_vp, _vp]),
    "awq_oneshot_ipc_open": (_i, [_vp, ctypes.POINTER(_vp)]),
    "awq_oneshot_ipc_close": (_i, [_vp]),
    "awq_oneshot_allreduce": (_i, [ctypes.POINTER(_vp), _vp, _vp, _i, _i, _i, _i, ctypes.c_uint, _i, _vp, _vp]),
    "awq_oneshot_allreduce_selftest": (_i, [ctypes.POINTER(_vp), _vp, _vp, _i, _i, _i, ctypes.c_uint, _i, _vp, _vp]),
    "awq_oneshot_allreduce_f32": (_i, [ctypes.POINTER(_vp), _vp, _vp, _i, _vp, _i, _i, _i, _i, ctypes.c_uint, _i, _vp, _vp]),
    "awq_oneshot_allreduce_f32_selftest": (_i, [ctypes.POINTER(_vp), _vp, _vp, _i, _vp, _i, _i, _i, ctypes.c_uint, _i, _vp, _vp]),
    "awq_oneshot_set_spin_limit": (_i, [ctypes.c_uint]),
    "awq_w4a16_partial_cdna4": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w3a16_partial": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "awq_w3a16_mlp_gate_up_forward_workspace_bytes": (_sz, [_i, _i, _i]),
    "awq_w3a16_mlp_gate_up_forward": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "awq_round_bias_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "awq_attn_decode_plan": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_decode_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "awq_attn_decode": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong,
                             ctypes.c_longlong, _i, _i, ctypes.c_float, ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_attn_prefill_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_prefill": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                              ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, _i, _i, _vp]),
    "awq_rope_kv_store": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _i, _vp]),
    "awq_attn_prefill_ftcache": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong,
                                      ctypes.c_float, _i, _i, _vp]),
    "awq_attn_splitkv_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_splitkv_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "awq_attn_splitkv": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                              ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_rope_kv_store_natural": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, _i,
                                       _vp]),
    "awq_rope_kv_store_natural_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong,
                                           ctypes.c_longlong, _i, _vp]),
    "awq_attn_prefill_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 10 + [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_splitkv_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 10 +
                             [ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_rope_kv_store_natural_pos": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong,
                                           ctypes.c_longlong, _i, _vp]),
    "awq_rope_kv_store_natural_pos_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, ctypes.c_longlong,
                                               ctypes.c_longlong, _i, _vp]),
    "awq_attn_kvcache_plan": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_kvcache_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "awq_attn_kvcache": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 6 +
                         [ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_attn_kvcache_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 10 +
                             [ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_rope_kv_store_paged_pos": (_i, [_vp] * 7 + [_i] * 10 + [ctypes.c_longlong] * 7 + [_i, _vp]),
    "awq_rope_kv_store_paged_pos_fp8": (_i, [_vp] * 9 + [_i] * 10 + [ctypes.c_longlong] * 11 + [_i, _vp]),
    "awq_attn_kvcache_paged": (_i, [_vp] * 5 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 6 +
                               [ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    "awq_attn_kvcache_paged_kv8": (_i, [_vp] * 7 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 10 +
                                   [ctypes.c_float, _i, _i, _vp, _sz, _vp]),
    # shared-prefix decode on the paged cache: the paged entries' arguments, then the group arrays and their four host ints
    "awq_attn_kvcache_shared_plan": (_i, [_i] * 7 + [ctypes.POINTER(_i)] * 4),
    "awq_attn_kvcache_shared_workspace_bytes": (_sz, [_i] * 7),
    "awq_attn_kvcache_paged_shared": (_i, [_vp] * 5 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 6 +
                                      [ctypes.c_float, _i, _i] + [_vp] * 3 + [_i, _i, ctypes.c_longlong, _i] + [_vp, _sz, _vp]),
    "awq_attn_kvcache_paged_shared_kv8": (_i, [_vp] * 7 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 10 +
                                          [ctypes.c_float, _i, _i] + [_vp] * 3 + [_i, _i, ctypes.c_longlong, _i] + [_vp, _sz, _vp]),
    "awq_kv_page_copy": (_i, [_vp] * 4 + [_i] * 5 + [ctypes.c_longlong] * 4 + [_vp]),
    "awq_kv_page_copy_fp8": (_i, [_vp] * 6 + [_i] * 5 + [ctypes.c_longlong] * 8 + [_vp]),
    "awq_attn_prefill_kvcache": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 6 + [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_kvcache_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _i] + [ctypes.c_longlong] * 10 +
                                     [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_paged": (_i, [_vp] * 5 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 6 +
                               [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_paged_kv8": (_i, [_vp] * 7 + [_i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 10 +
                                   [ctypes.c_float, _i, _i, _vp]),
    # packed steps (per-sequence query lengths): cu_seqlens_q, max_seqlen_q, total_q in the place of one seqlen
    "awq_attn_varq_plan": (_i, [_i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_prefill_kvcache_varq": (_i, [_vp] * 4 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_kvcache_varq_kv8": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 9 +
                                          [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_paged_varq": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                    [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_prefill_paged_varq_kv8": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                        [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i, _vp]),
    "awq_attn_varq_split_plan": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_varq_split_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    # the four packed one-pass entries' arguments with (split_seqlen_q, split_min_keys, workspace, workspace_bytes) in front of the stream
    "awq_attn_varq": (_i, [_vp] * 4 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i] +
                      [_i, _i, _vp, _sz, _vp]),
    "awq_attn_varq_kv8": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i] +
                          [_i, _i, _vp, _sz, _vp]),
    "awq_attn_paged_varq": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 5 +
                            [ctypes.c_float, _i, _i] + [_i, _i, _vp, _sz, _vp]),
    "awq_attn_paged_varq_kv8": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 + [ctypes.c_longlong] * 9 +
                                [ctypes.c_float, _i, _i] + [_i, _i, _vp, _sz, _vp]),
    # a sliding window on a mixed step: awq_attn_varq*'s arguments with window_left behind split_min_keys
    "awq_attn_varq_window_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_varq_window_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "awq_attn_varq_window": (_i, [_vp] * 4 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i] +
                             [_i, _i, _i, _vp, _sz, _vp]),
    "awq_attn_varq_window_kv8": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i] +
                                 [_i, _i, _i, _vp, _sz, _vp]),
    "awq_attn_paged_varq_window": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                   [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i] + [_i, _i, _i, _vp, _sz, _vp]),
    "awq_attn_paged_varq_window_kv8": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                       [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i] + [_i, _i, _i, _vp, _sz, _vp]),
    # capped logits on a windowed mixed step: the *_window entries' arguments with softcap behind window_left
    "awq_attn_varq_softcap": (_i, [_vp] * 4 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i] +
                              [_i, _i, _i, ctypes.c_float, _vp, _sz, _vp]),
    "awq_attn_varq_softcap_kv8": (_i, [_vp] * 6 + [_i, _vp, _i, _i, _vp] + [_i] * 6 + [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i] +
                                  [_i, _i, _i, ctypes.c_float, _vp, _sz, _vp]),
    "awq_attn_paged_varq_softcap": (_i, [_vp] * 5 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                    [ctypes.c_longlong] * 5 + [ctypes.c_float, _i, _i] + [_i, _i, _i, ctypes.c_float, _vp, _sz, _vp]),
    "awq_attn_paged_varq_softcap_kv8": (_i, [_vp] * 7 + [_i, _vp, _i, _i, _vp] + [_i] * 5 + [ctypes.c_longlong] + [_i] * 3 +
                                        [ctypes.c_longlong] * 9 + [ctypes.c_float, _i, _i] + [_i, _i, _i, ctypes.c_float, _vp, _sz, _vp]),
    "awq_rope_kv_store_natural_varq": (_i, [_vp] * 6 + [_i, _i, _vp] + [_i] * 8 + [ctypes.c_longlong, _i, _vp]),
    "awq_rope_kv_store_natural_varq_fp8": (_i, [_vp] * 8 + [_i, _i, _vp] + [_i] * 8 + [ctypes.c_longlong, _i, _vp]),
    "awq_rope_kv_store_paged_varq": (_i, [_vp] * 7 + [_i, _vp] + [_i] * 10 + [ctypes.c_longlong] * 6 + [_i, _vp]),
    "awq_rope_kv_store_paged_varq_fp8": (_i, [_vp] * 9 + [_i, _vp] + [_i] * 10 + [ctypes.c_longlong] * 10 + [_i, _vp]),
    "awq_attn_varlen_plan": (_i, [_i, _i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_attn_varlen": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, ctypes.c_longlong, _i, _i, ctypes.c_longlong, ctypes.c_longlong,
                             ctypes.c_longlong, ctypes.c_float, _i, _i, _vp]),
    "awq_rope_with_pos": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong,
                               ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _i, _vp]),
    "awq_rope_neox_inplace": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "awq_w8a8_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "awq_w8a8_gemm_plan": (_i, [_i, _i, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "awq_quant_per_token": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "awq_gelu_quant_per_token": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp]),
    "awq_layernorm_quant": (_i, [_vp, _vp, _vp, ctypes.c_float, _vp, _vp, _i, _i, _i, _i, _vp]),
    "awq_tune_set": (_i, [ctypes.c_char_p, _i]),
}
# the _qknorm sibling of every natural-layout store: its arguments with q_gamma, k_gamma and norm_eps directly after the angles
for _n in ("natural", "natural_pos", "paged_pos", "natural_varq", "paged_varq"):
    for _f in ("", "_fp8"):
        _args = SIGNATURES["awq_rope_kv_store_" + _n + _f][1]
        SIGNATURES["awq_rope_kv_store_" + _n + _f + "_qknorm"] = (_i, _args[:2] + [_vp, _vp, ctypes.c_float] + _args[2:])


class AwqNativeError(RuntimeError):
    pass


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AwqNativeError(
                f"{LIB_PATH} is missing: the MI355X HIP library has not been built "
                "(run `python -m llm_awq_amd.build`). There is no CPU/PyTorch fallback for the hot path.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if L.awq_abi_version() != 1:
            raise AwqNativeError("libawq_cdna4.so ABI version mismatch")
        _lib = L
    return _lib


def check(status: int) -> None:
    if status != 0:
        L = lib()
        msg = L.awq_status_string(status).decode()
        if status == -8:
            msg += " " + L.awq_last_hip_error().decode()
        raise AwqNativeError(f"awq_cdna4 error {status}: {msg}")


def tune(**knobs) -> None:
    """awq_tune_set for each knob (tests, experiments and benchmarks only: opts this process in with AWQ_TUNING=1)."""
    os.environ["AWQ_TUNING"] = "1"
    for k, v in knobs.items():
        check(lib().awq_tune_set(k.encode(), int(v)))
