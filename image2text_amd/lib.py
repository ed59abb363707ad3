"""ctypes binding of libi2t_hip.so (include/i2t.h).  Loading fails loudly: there is no fallback path."""
import ctypes as C
import os

import torch  # must come first: libi2t_hip.so has to bind to the HIP runtime torch has already loaded

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('I2T_LIB') or os.path.join(_HERE, 'csrc', 'libi2t_hip.so')      # I2T_LIB: A/B builds of the same ABI

P, I, L, F, I64, U = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_int64, C.c_uint


# Pointer kinds: P is void*, each subclass a pointer to one element type.  As an argtype a subclass takes what c_void_p takes (an
# address or None), so binding the table below as argtypes is unchanged by them.  The docstring is the C type, for error texts.
class PF(P):
    """float*"""


class PI(P):
    """int*"""


class PL(P):
    """int64_t*"""


class PN(P):          # 64 bits wherever the library builds
    """long*"""


class PU(P):          # the two 32-bit words of a seed, kept in an int32 tensor
    """unsigned*"""


# kind -> the torch dtype a tensor behind it must have; None: any (bf16, e4m3 bytes, or f32-or-bf16 behind an *_is_f32 flag)
POINTER_DTYPE = {P: None, PF: torch.float32, PI: torch.int32, PL: torch.int64, PN: torch.int64, PU: torch.int32}

# name -> argtypes, in the order of include/i2t.h.  A pointer's kind says what the header declares behind it; ops.py's checked caller
# reads the kinds of an entry point with a leading stream and refuses, before the call, an operand that is not on the device or has
# another dtype than its kind's (POINTER_DTYPE).  tests/test_abi.py holds every row to the header, pointee for pointee.
SIGNATURES = {
    'i2t_abi_version': [],
    'i2t_last_error': [C.c_char_p, C.c_size_t],
    'i2t_gemm_bf16': [P, P, I, I, P, I, I, P, I, I, I, I, I, F, PF, I, P, I, P, I, PF, I, I, I, U, U, F],
    'i2t_gemm_bf16_ex': [P, P, I, I, P, I, I, P, I, I, I, I, I, F, PF, I, P, I, P, I, PF, I, I, I, U, U, F, PF],
    'i2t_gemm_reserve_cus': [I],
    'i2t_gemm_reserved_cus': [],
    'i2t_xattn_kv_fused': [P, P, I, P, I, PF, P, L, I, PI, I, P, I, P, L, I, PF, I, I, I, I, U, U, F],
    'i2t_colsum_bf16': [P, P, I, I, I, PF, I],
    'i2t_colsum_bf16_ex': [P, P, I, I, I, PF, I, PF],
    'i2t_gemm_dw_colsum_bf16': [P, P, I, P, I, PF, I, I, I, I, F, PF, PF],
    'i2t_layernorm_fwd': [P, PF, PF, PF, P, I, PF, PF, I, I],
    'i2t_layernorm_fwd_eps': [P, PF, PF, PF, P, I, PF, PF, I, I, F],
    'i2t_layernorm_bwd': [P, P, I, PF, PF, PF, PF, PF, I, P, PF, PF, I, I, U, U, F, PF, PF],
    'i2t_layernorm_bwd_ex': [P, P, I, PF, PF, PF, PF, PF, I, P, PF, PF, I, I, U, U, F, PF, PF, U, U, F, I, I],
    'i2t_layernorm_nd_fwd': [P, PF, PF, PF, PF, PF, L, PF, I, I, I],
    'i2t_layernorm_nd_fwd_drop': [P, PF, PF, PF, PF, PF, L, PF, I, I, I, U, U, F, L],
    'i2t_layernorm_nd_bwd': [P, PF, L, PF, PF, PF, PF, PF, PF, PF, PF, I, I, I],
    'i2t_attention_fwd': [P, P, L, I, P, L, I, P, L, I, P, L, I, PF, I, I, I, I, I, U, U, F, PI, PI, I],
    'i2t_attention_bwd': [P, P, L, I, P, L, I, P, L, I, P, L, I, P, L, I, PF, PF, P, L, I, P, L, I, P, L, I, I, I, I, I, I, U, U, F, PI, PI, I, U, U,
                          F],
    'i2t_attention_bwd_ex': [P, P, L, I, P, L, I, P, L, I, P, L, I, P, L, I, PF, PF, P, L, I, P, L, I, P, L, I, I, I, I, I, I, U, U, F, PI, PI, I, U,
                             U, F, I],
    'i2t_embed_fwd': [P, PL, PF, PF, PF, I, I, I, I, I, PI],
    'i2t_embed_bwd': [P, PL, PF, PF, PF, I, I, I, I, I, PI],
    'i2t_ce_fwd': [P, P, I, PL, PF, F, I64, PF, PF, I, I],
    'i2t_ce_bwd': [P, P, I, PL, PF, F, I64, PF, PF, I, I],
    'i2t_ce_fwd_bwd': [P, P, I, PL, PF, F, I64, PF, PF, I, I],
    'i2t_scale_bf16': [P, P, L, PF],
    'i2t_ce_distill_fwd': [P, P, I, P, I, F, PL, PF, F, I64, PF, PF, PF, I, I],
    'i2t_ce_distill_bwd': [P, P, I, P, I, F, PL, PF, F, I64, PF, PF, PF, I, I],
    'i2t_ema_update': [P, PF, PF, P, L, F],
    'i2t_lm_inputs': [P, PL, PL, I, I, I64, I64, I64, I, I64, F, F, U, U],
    'i2t_grad_normalize': [P, PF, L, PF, P, U, U, F, I, PF],
    'i2t_conv_fwd': [P, P, I, I, PF, PF, P, PF, I, I, I, I, I, I],
    'i2t_conv_bwd_data': [P, P, PF, P, I, P, PF, I, I, I, I, I, I],
    'i2t_conv_bwd_weight': [P, P, P, I, I, PF, PF, I, I, I, I, I, I],
    'i2t_conv6_fwd': [P, P, I, I, PF, PF, P, I, P, I, I, I, I, I],
    'i2t_conv6_bwd_data': [P, P, I, PF, P, P, P, I, I, I, I, I],
    'i2t_conv6_bwd_weight': [P, P, I, P, I, I, PF, PF, PF, I, I, I, I, I],
    'i2t_nchw_to_nhwc_bf16': [P, P, P, I, I, I, I],
    'i2t_cast_f32_bf16': [P, PF, P, L],
    'i2t_split_f32_bf16': [P, PF, P, P, L, I],
    'i2t_dropout_apply': [P, P, I, L, I, I, U, U, F],
    'i2t_adamw_step': [P, PF, PF, PF, PF, P, L, PN, PF, PF, I, F, F, F, I, F],
    'i2t_snradam_step': [P, PF, PF, PF, PF, P, L, PN, PF, PF, I, F, F, F, I, F],
    'i2t_bcast_rows': [P, PF, PF, L, I, I, I],
    'i2t_bcast_rows_drop': [P, PF, PF, L, I, I, I, U, U, F],
    'i2t_sum_over_batch': [P, PF, L, PF, I, I, I, I],
    'i2t_copy_rows': [P, PF, L, P, L, I, I, I, I],
    'i2t_add_f32': [P, PF, PF, L],
    'i2t_decode_attention': [P, P, I, P, P, L, I, L, P, I, PI, I, I, I, I],
    'i2t_kv_append': [P, P, I, P, P, L, I, PI, I, I],
    'i2t_kv_prefill': [P, P, I, I, I, I, I, I, P, P, L, I, L, I, I, I, I, I],
    'i2t_ngram_ban_argmax': [P, P, I, I, PL, I, PI, PI, I, I, I, PF],
    'i2t_gemm_bf16_top2': [P, P, I, P, I, I, I, I, PF, I],
    'i2t_top2_ngram_argmax': [P, PF, I, P, I, P, I, I, PL, I, PI, PI, I, I, I],
    'i2t_sample_token': [P, PF, I, PL, I, PI, PI, I, I, I, F, I, F, PU, PF, I],
    'i2t_gemm_bf16_lse': [P, P, I, P, I, I, I, I, F, PF, I],
    'i2t_lse_token_logprob': [P, PF, I, P, I, P, I, I, F, PL, I64, PF, PF, I, I],
    'i2t_embed_step': [P, PL, I, PI, PF, PF, PF, I, I, I, I],
    'i2t_advance': [P, PI, I, I],
    'i2t_gemm_bf16_top2_lse': [P, P, I, P, I, I, I, I, PF, PF, I],
    'i2t_top2_ngram_argmax_lp': [P, PF, PF, I, P, I, P, I, I, PL, I, PI, PI, I, I, I, PI, PF, I],
    'i2t_ngram_ban_argmax_lp': [P, PF, I, PL, I, PI, PI, I, I, I, PI, PF, I],
    'i2t_sample_token_lp': [P, PF, I, PL, I, PI, PI, I, I, I, F, I, F, PU, PF, I, PI, PF, I],
    'i2t_caption_finish': [P, PL, I, PI, I, I64, PI, PI, PF, I, PI, I],
    'i2t_caption_finish_ragged': [P, PL, I, PI, PL, I, PI, I, I, I, I64, PI, PI, PF, I, PI, I],
    'i2t_caption_logits_process': [P, PF, I, PL, I, PI, PI, I, I, PI, I, I, I, F, F, PI, PF, PF, I, I, I],
    'i2t_caption_raw_logprob': [P, PL, I, PI, PF, PF, I, PF, I, PI, PF, I, I, I],
    'i2t_caption_top_logprobs': [P, PF, I, PI, PI, I, PI, PI, PI, PF, PF, I, I, I, I],
    'i2t_score_top_logprobs': [P, PF, I, F, PL, I64, PI, PF, PF, PI, PF, PF, I, I, I],
    'i2t_caption_trie_mask': [P, PF, I, PI, PI, PI, PI, I, I, I, PI, PF, PF, I, I, I],
    'i2t_caption_trie_advance': [P, PL, I, PI, PI, PF, I, PF, PI, PI, PI, PI, I, I, I, PI, PI, PI, PF, I, I, I],
    'i2t_rows_lse': [P, PF, I, PF, I, I],
    'i2t_trie_level_expand': [P, P, I, P, I, I, F, PF, I, PF, PF, PF, PI, PI, I, PI, PI, PI, I, I, PL, I, PI, PF, I, I, I, I, I],
    'i2t_trie_level_expand_sets': [P, P, I, P, I, I, F, PF, I, PF, PF, PF, PI, PI, I, PI, I, PI, I, PI, I, PI, I, I, PL, I, PF, I, I, I, I, I,
                                   I],
    'i2t_trie_beam_candidates': [P, PF, I, PI, PF, PI, PI, PI, I, I, I, PI, PI, PF, PF, PF, I, I, I],
    'i2t_trie_beam_select': [P, PI, PF, PF, PI, PF, PI, PI, PI, I, I, I, PL, I, PI, I, PI, PF, PF, PI, PI, PI, PI, PI, PI, I, I, I, I, F],
    'i2t_caption_trie_mask_ragged': [P, PF, I, PI, PI, PI, PI, I, I, I, PI, PF, PF, I, PI, PI, I, I, I],
    'i2t_caption_trie_advance_ragged': [P, PL, I, PI, PI, PF, I, PF, PI, PI, PI, PI, I, I, I, PI, PI, PI, PF, I, PI, I, I, I],
    'i2t_trie_beam_select_sets': [P, PI, PF, PF, PI, PF, PI, PI, PI, I, I, I, PL, I, PI, I, PI, PF, PF, PI, PI, PI, PI, PI, PI, I, I, I, PI, PI,
                                  F],
    'i2t_gq_attention_fwd': [P, P, L, I, P, L, I, P, L, I, P, L, I, PF, I, I, I, I, I, I, I, U, U, F, PI, PI, I, I],
    'i2t_gq_attention_bwd': [P, P, L, I, P, L, I, P, L, I, P, L, I, P, L, I, PF, PF, P, L, I, P, L, I, P, L, I, I, I, I, I, I, I, I, U, U, F, PI, PI,
                             I, U, U, F],
    'i2t_row_sections_dropout': [P, P, I, L, I, I, U, U, F],
    'i2t_gather_rows': [P, PF, PI, PF, P, L, I],
    'i2t_scatter_rows': [P, PF, PI, PF, L, I],
    'i2t_moe_gate_fwd': [P, PF, I, PF, PF, P, I, PF, PF, I, I, I, I, I, F],
    'i2t_moe_gate_bwd_blocks': [I],
    'i2t_moe_gate_bwd': [P, P, I, PF, I, PF, PF, PF, P, I, PF, PF, PF, I, I, I, I, I, F],
    'i2t_moe_pack_w2': [P, P, PF, P, I, I, I, I],
    'i2t_moe_unpack_dw2': [P, PF, PF, PF, I, I, I, I],
    'i2t_gq_decode_attention': [P, P, I, P, P, I, P, P, L, I, P, I, PI, I, I, I, I, I, I],
    'i2t_gq_decode_attention_long': [P, P, I, P, P, I, P, P, L, I, P, I, PI, I, I, I, I, I, I, PF, L],
    'i2t_beam_gq_decode_attention_long': [P, P, I, P, P, I, P, P, L, I, P, I, PI, I, I, PI, I, I, I, I, I, PF, L],
    'i2t_beam_candidates': [P, PF, I, PL, I, PI, PI, PI, I, I, I, I, F, I, I, F, PU, PI, PF, PI],
    'i2t_beam_consolidate': [P, PI, PF, PF, PL, I, PI, I, PI, PI, PI, PI, PI, I, I, I, F, I, PU, PI],
    'i2t_beam_pool_select': [P, PI, PF, PF, PL, I, PI, I, PF, I, PL, PF, PF, PF, PI, PI, PI, PI, PI, PI, I, I, I, I, I, I, F, I],
    'i2t_beam_advance': [P, PI, PI],
    'i2t_beam_decode_attention': [P, P, I, P, P, L, I, L, P, I, PI, I, I, PI, I, I, I, I],
    'i2t_beam_gq_decode_attention': [P, P, I, P, P, I, P, P, L, I, P, I, PI, I, I, PI, I, PI, I, I, I, I, I],
    'i2t_mem_decode_attention': [P, P, I, P, P, L, I, P, I, I, PI, I, I, I],
    'i2t_mem_gq_decode_attention': [P, P, I, P, P, L, I, P, I, I, PI, I, I, I, I, I],
    'i2t_sparse_step_setup': [P, PI, PI, PI, PI, PI, I, I],
    'i2t_select_rows': [P, PI, PF, PF, PF, L],
    'i2t_grouped_gemm': [P, I, P, I, P, I, L, P, I, L, I, PF, L, I, P, P, I, PF, I, I, PI, I, I, PI, I, I, I],
    'i2t_grouped_colsum': [P, P, I, PI, I, PF, L, I, I],
    'i2t_sumsq': [P, PF, L, PF, I],
    'i2t_rmsnorm_fwd': [P, PF, PF, P, PF, PF, I, I, F],
    'i2t_rmsnorm_bwd': [P, P, I, PF, PF, PF, PF, I, P, PF, I, I],
    'i2t_rope': [P, P, I, I, I, I, PF, I, PI, PI, I, I, I, I],
    'i2t_swiglu_fwd': [P, P, I, P, I, I],
    'i2t_swiglu_bwd': [P, P, P, I, P, I, I],
    'i2t_dgelu_mul': [P, PF, P, P, L],
    'i2t_dgelu_erf_mul': [P, PF, P, P, L],
    'i2t_gelu_fwd': [P, P, P, L, I],
    'i2t_lora_stage': [P, P, P, I, P, L, I, U, U, F],
    'i2t_gemm_bf16_ws': [P, P, I, P, I, P, I, I, I, I, I, PF, I, PF, I, PF, L],
    'i2t_patchify': [P, PF, P, I, I, I, I, I],
    'i2t_vit_tokens': [P, PF, PF, PF, PF, I, I, I],
    'i2t_l2norm_fwd': [P, PF, PF, P, PF, I, I],
    'i2t_l2norm_bwd': [P, PF, PF, PF, PF, I, I, I],
    'i2t_transpose_last2': [P, PF, PF, P, L, I, I],
    'i2t_peer_lookup_fwd': [P, PF, P, PF, P, P, PF, PI, PI, PF, PF, I, I, I, I, I, I],
    'i2t_peer_lookup_bwd': [P, PF, P, P, P, PI, PI, PF, PF, PF, P, PF, PF, I, I, I, I, I, I],
    'i2t_gemm_f32': [P, PF, PF, PF, I, I, I],
    'i2t_lsh_embed_fwd': [P, PF, PF, L, PN, PI, PF, PI, PF, PI, I, I, I, I, I],
    'i2t_lsh_embed_bwd': [P, PF, PI, PF, L, PN, I, I, I, I, I],
    'i2t_l2norm_groups_fwd': [P, PF, PN, PF, PF, I, I, I],
    'i2t_l2norm_groups_bwd': [P, PF, PF, PN, PF, PF, I, I, I, I],
    'i2t_lsh_soft_fwd': [P, PF, PF, L, PN, PI, PI, P, PF, I, I, I, I, I],
    'i2t_lsh_soft_bwd': [P, PF, PF, PF, PF, PF, L, PN, PI, PI, PF, PF, I, I, I, I, I],
    'i2t_quant_rows_fp8': [P, P, I, I, P, I, PF, I, I],
    'i2t_quant_cols_fp8': [P, P, I, P, I, PF, I, I],
    'i2t_rmsnorm_fwd_fp8': [P, PF, PF, P, I, PF, PF, I, I, F, P],
    'i2t_swiglu_fwd_fp8': [P, P, I, P, I, PF, I, I, P],
    'i2t_swiglu_bwd_fp8': [P, P, P, I, P, I, PF, I, I, P],
    'i2t_gemm_fp8': [P, P, I, PF, P, I, PF, P, I, I, I, I, I, PF, I, PF, I],
    'i2t_preprocess_images': [P, P, L, PL, PI, I, I, PF, I, I, F, F, F, F, F, F, I],
    'i2t_preprocess_regions': [P, P, L, PL, PI, I, I, PI, I, PF, I, I, F, F, F, F, F, F, I],
    'i2t_set_deterministic': [I],
    'i2t_deterministic': [],
    'i2t_comm_available': [],
    'i2t_comm_unique_id': [P, I],
    'i2t_comm_init': [P, I, I, C.POINTER(C.c_void_p)],
    'i2t_comm_allreduce': [P, P, PF, L, I, P],
    'i2t_comm_destroy': [P],
    'i2t_workspace_bytes': [C.c_char_p, L, L, L, PN],
    'i2t_graph_capture_begin': [P],
    'i2t_graph_capture_end': [P, C.POINTER(C.c_void_p)],
    'i2t_graph_launch': [P, P],
    'i2t_graph_destroy': [P],
}

ABI_VERSION = 22
_lib = None


class I2TError(RuntimeError):
    pass


def load():
    """Load the shared library once; raise if it is missing (build with ``python -m image2text_amd.build``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise I2TError(f'{LIB_PATH} not found: the HIP extension is required (python -m image2text_amd.build); '
                       'there is no CPU or eager fallback for the hot path')
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.argtypes = argtypes
        fn.restype = C.c_int
    if lib.i2t_abi_version() != ABI_VERSION:
        raise I2TError(f'ABI version mismatch: library {lib.i2t_abi_version()} vs binding {ABI_VERSION}')
    _lib = lib
    return lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    load().i2t_last_error(buf, 512)
    return buf.value.decode(errors='replace')


def check(rc: int, what: str = ''):
    if rc != 0:
        raise I2TError(f'{what or "i2t call"} failed (rc={rc}): {last_error()}')
