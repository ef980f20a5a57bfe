"""Python host side of the MI355X embedding engine.

* ``BertModel`` mirrors the reference's ctypes client (examples/sample_dylib.py:17-62:
  same constructor argument, ``n_embd``, ``encode(sentences, batch_size=16)``) on top of
  the C ABI of ``build/libbert.so`` -- the library does all the work (tokenizer, HIP
  kernels, multi-GPU sharding); this module only marshals pointers.
* ``load_lib`` declares argtypes for every symbol of include/bert.h and
  include/bert_hip.h.
* ``write_model`` / ``synthetic_model`` write model files in the reference's format
  (reference bert.cpp:434-766, models/convert-to-ggml.py:68-108) so a GPU box with no
  checkpoints can build the BASELINE architectures from a seed.
"""
import ctypes
import os
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# BERT_LIB: another build of the same library (A/B measurements)
LIB_PATH = os.environ.get("BERT_LIB") or os.path.join(ROOT, "build", "libbert.so")

FTYPE = {"f32": 0, "f16": 1, "q4_0": 2, "q4_1": 3, "q8_0": 8}

_lib = None

c_i32 = ctypes.c_int32
c_f32p = ctypes.POINTER(ctypes.c_float)
c_i32p = ctypes.POINTER(ctypes.c_int32)


def load_lib(path=None):
    """Load libbert.so once and declare its ABI.  Raises if the build is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(f"{p} not built: run `make -C embeddings.cpp_amd` (or __graft_entry__.build())")
    L = ctypes.CDLL(p)
    vp = ctypes.c_void_p
    L.bert_load_from_file.restype = vp
    L.bert_load_from_file.argtypes = [ctypes.c_char_p]
    L.bert_free.argtypes = [vp]
    L.bert_n_embd.restype = c_i32
    L.bert_n_embd.argtypes = [vp]
    L.bert_n_max_tokens.restype = c_i32
    L.bert_n_max_tokens.argtypes = [vp]
    L.bert_vocab_id_to_token.restype = ctypes.c_char_p
    L.bert_vocab_id_to_token.argtypes = [vp, c_i32]
    L.bert_tokenize.argtypes = [vp, ctypes.c_char_p, c_i32p, c_i32p, c_i32]
    L.bert_encode.argtypes = [vp, c_i32, ctypes.c_char_p, c_f32p]
    L.bert_encode_batch.argtypes = [vp, c_i32, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p),
                                    ctypes.POINTER(c_f32p)]
    L.bert_forward.argtypes = [vp, c_i32, c_i32p, c_i32, c_f32p]
    for fn in (L.bert_forward_batch, L.bert_forward_fake_batch):
        fn.argtypes = [vp, c_i32, c_i32, ctypes.POINTER(c_i32p), c_i32p, ctypes.POINTER(c_f32p)]
    L.bertx_num_devices.restype = c_i32
    L.bertx_num_devices.argtypes = [vp]
    L.bertx_device_ordinal.restype = c_i32
    L.bertx_device_ordinal.argtypes = [vp, c_i32]
    L.bertx_hparams.argtypes = [vp, c_i32p]
    L.bertx_forward_device.restype = c_i32
    L.bertx_forward_device.argtypes = [vp, c_i32, vp, vp, c_i32, c_i32, c_i32, vp, vp]
    L.bertx_reserve.restype = c_i32
    L.bertx_reserve.argtypes = [vp, c_i32, c_i32, c_i32]
    L.bertx_set_profiling.argtypes = [vp, c_i32]
    L.bertx_reset_stats.argtypes = [vp]
    L.bertx_kernel_stats.restype = c_i32
    L.bertx_kernel_stats.argtypes = [vp, c_i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int64),
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), c_i32p]
    L.bertx_device_last_call.restype = c_i32
    L.bertx_device_last_call.argtypes = [vp, c_i32, ctypes.POINTER(ctypes.c_double), c_i32p,
                                         ctypes.POINTER(ctypes.c_int64)]
    L.bertx_device_calls.restype = ctypes.c_int64
    L.bertx_device_calls.argtypes = [vp, c_i32]
    L.bertx_quantize_file.restype = c_i32
    L.bertx_quantize_file.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_i32]
    L.bertx_convert_hf.restype = c_i32
    L.bertx_convert_hf.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_i32]
    L.bertx_test_gemm.restype = c_i32
    L.bertx_test_attention.restype = c_i32
    L.bertx_test_attention.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp]
    L.bertx_test_gemm.argtypes = [c_i32, c_i32, c_i32, vp, c_f32p, c_i32, vp, c_i32, vp, vp, c_i32]
    L.bertx_test_gemm_ln.restype = c_i32
    L.bertx_test_gemm_ln.argtypes = [c_i32, c_i32, c_i32, vp, vp, c_i32, vp, vp, vp, vp, c_i32] + [vp] * 7 + [c_i32]
    try:   # (absent from libraries built before it: BERT_LIB A/B runs against older builds)
        L.bertx_test_gemm_fold.restype = c_i32
        L.bertx_test_gemm_fold.argtypes = [c_i32, c_i32, c_i32, vp, vp, c_i32, vp, vp, vp, vp, c_i32, vp, vp, vp, c_i32]
    except AttributeError:
        pass
    try:   # (the launched-row-count forms: absent from older BERT_LIB builds)
        L.bertx_test_gemm_rows.restype = c_i32
        L.bertx_test_gemm_rows.argtypes = ([c_i32, c_i32, c_i32, vp, vp, c_i32, c_i32, vp, vp, vp, vp, c_i32] +
                                           [vp] * 5 + [c_i32, vp, vp, vp, c_i32])
        L.bertx_test_gemm_fold_rows.restype = c_i32
        L.bertx_test_gemm_fold_rows.argtypes = [c_i32, c_i32, c_i32, vp, vp, c_i32, c_i32, vp, vp, vp, vp, c_i32, vp, vp,
                                                vp, c_i32]
        L.bertx_test_cu_count.restype = c_i32
        L.bertx_test_cu_count.argtypes = []
    except AttributeError:
        pass
    L.bertx_test_gemm_ran.restype = c_i32
    L.bertx_test_gemm_ran.argtypes = []
    L.bertx_test_gemm_f32.restype = c_i32
    L.bertx_test_gemm_f32.argtypes = [c_i32, c_i32, vp, vp, c_i32, vp, c_i32, vp, vp]
    try:   # (the activation mode and its hooks: absent from older BERT_LIB builds)
        L.bertx_load_from_file.restype = vp
        L.bertx_load_from_file.argtypes = [ctypes.c_char_p, c_i32]
        L.bertx_activation_mode.restype = c_i32
        L.bertx_activation_mode.argtypes = [vp]
        L.bertx_test_quantize_act.restype = c_i32
        L.bertx_test_quantize_act.argtypes = [c_i32, c_i32, c_i32, vp, vp, vp, vp]
        L.bertx_test_gemm_q8.restype = c_i32
        L.bertx_test_gemm_q8.argtypes = [c_i32, c_i32, c_i32, vp, vp, c_i32, vp, c_i32, vp, vp]
    except AttributeError:
        pass
    try:   # (pooling modes and per-token output: absent from older BERT_LIB builds)
        L.bertx_set_pooling.restype = c_i32
        L.bertx_set_pooling.argtypes = [vp, c_i32]
        L.bertx_pooling.restype = c_i32
        L.bertx_pooling.argtypes = [vp]
        L.bertx_set_cls_pruning.restype = c_i32
        L.bertx_set_cls_pruning.argtypes = [vp, c_i32]
        L.bertx_forward_tokens.restype = c_i32
        L.bertx_forward_tokens.argtypes = [vp, c_i32, ctypes.POINTER(c_i32p), c_i32p, ctypes.POINTER(c_f32p)]
        L.bertx_forward_tokens_device.restype = c_i32
        L.bertx_forward_tokens_device.argtypes = [vp, c_i32, vp, vp, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_test_attention_cls.restype = c_i32
        L.bertx_test_attention_cls.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp]
    except AttributeError:
        pass
    try:   # (the row-kernel parity hooks: absent from older BERT_LIB builds)
        L.bertx_test_embed_ln.restype = c_i32
        L.bertx_test_embed_ln.argtypes = [c_i32] * 7 + [vp] * 7 + [c_i32, c_i32, vp, vp, c_i32]
        L.bertx_test_ln_stats.restype = c_i32
        L.bertx_test_ln_stats.argtypes = [vp, c_i32, c_i32, c_i32, c_i32, vp, c_i32]
        L.bertx_test_pool.restype = c_i32
        L.bertx_test_pool.argtypes = [c_i32, vp, vp, vp, vp, vp, c_i32, c_i32, c_i32, c_i32, vp, c_i32]
        L.bertx_test_f32_rows.restype = c_i32
        L.bertx_test_f32_rows.argtypes = [c_i32, vp, vp, c_i32, c_i32, vp, vp, c_i32, vp, c_i32]
        L.bertx_test_attention_f32.restype = c_i32
        L.bertx_test_attention_f32.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32]
    except AttributeError:
        pass
    try:   # (which attention kernel ran, the CLS gather hook: absent from older BERT_LIB builds)
        L.bertx_test_attention_ran.restype = c_i32
        L.bertx_test_attention_ran.argtypes = []
        L.bertx_test_attention_cls_gather.restype = c_i32
        L.bertx_test_attention_cls_gather.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp, vp, vp, vp, vp]
    except AttributeError:
        pass
    try:   # (the embedding index: absent from older BERT_LIB builds)
        L.bertx_index_create.restype = vp
        L.bertx_index_create.argtypes = [vp, c_i32, c_i32]
        L.bertx_index_create_ex.restype = vp
        L.bertx_index_create_ex.argtypes = [vp, c_i32, c_i32, c_i32]
        L.bertx_index_storage.restype = c_i32
        L.bertx_index_storage.argtypes = [vp]
        L.bertx_index_rows_i8.restype = c_i32
        L.bertx_index_rows_i8.argtypes = [vp, c_i32, c_i32, vp, vp]
        L.bertx_index_free.restype = None
        L.bertx_index_free.argtypes = [vp]
        for fn in (L.bertx_index_clear, L.bertx_index_size, L.bertx_index_capacity, L.bertx_index_dim):
            fn.restype = c_i32
            fn.argtypes = [vp]
        L.bertx_index_add.restype = c_i32
        L.bertx_index_add.argtypes = [vp, vp, c_i32]
        L.bertx_index_add_device.restype = c_i32
        L.bertx_index_add_device.argtypes = [vp, vp, c_i32, vp]
        L.bertx_index_rows.restype = c_i32
        L.bertx_index_rows.argtypes = [vp, c_i32, c_i32, vp]
        L.bertx_index_search.restype = c_i32
        L.bertx_index_search.argtypes = [vp, vp, c_i32, c_i32, vp, vp]
        L.bertx_index_search_device.restype = c_i32
        L.bertx_index_search_device.argtypes = [vp, vp, c_i32, c_i32, vp, vp, vp]
        L.bertx_index_add_texts.restype = c_i32
        L.bertx_index_add_texts.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p)]
        L.bertx_index_search_texts.restype = c_i32
        L.bertx_index_search_texts.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32, vp, vp]
        L.bertx_bench_search.restype = c_i32
        L.bertx_bench_search.argtypes = [c_i32] * 5 + [c_f32p]
        L.bertx_bench_search_add_rate.restype = c_i32
        L.bertx_bench_search_add_rate.argtypes = [c_i32, c_i32, ctypes.POINTER(ctypes.c_double)]
        L.bertx_bench_search_ex.restype = c_i32
        L.bertx_bench_search_ex.argtypes = [c_i32] * 6 + [c_f32p]
        L.bertx_bench_search_add_rate_ex.restype = c_i32
        L.bertx_bench_search_add_rate_ex.argtypes = [c_i32, c_i32, c_i32, ctypes.POINTER(ctypes.c_double)]
    except AttributeError:
        pass
    try:   # (binary storage, listed rows, the rescored search: absent from older BERT_LIB builds)
        L.bertx_index_rows_bits.restype = c_i32
        L.bertx_index_rows_bits.argtypes = [vp, c_i32, c_i32, vp]
        L.bertx_index_score_ids.restype = c_i32
        L.bertx_index_score_ids.argtypes = [vp, vp, c_i32, vp, c_i32, vp]
        L.bertx_index_score_ids_device.restype = c_i32
        L.bertx_index_score_ids_device.argtypes = [vp, vp, c_i32, vp, c_i32, vp, vp]
        L.bertx_index_search_rescored.restype = c_i32
        L.bertx_index_search_rescored.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_index_search_rescored_device.restype = c_i32
        L.bertx_index_search_rescored_device.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, vp, vp, vp]
        L.bertx_index_remove.restype = c_i32
        L.bertx_index_remove.argtypes = [vp, vp, c_i32]
        L.bertx_index_remove_device.restype = c_i32
        L.bertx_index_remove_device.argtypes = [vp, vp, c_i32, vp]
        L.bertx_index_live.restype = c_i32
        L.bertx_index_live.argtypes = [vp]
        L.bertx_index_deleted.restype = c_i32
        L.bertx_index_deleted.argtypes = [vp, c_i32, c_i32, vp]
        L.bertx_index_search_filtered.restype = c_i32
        L.bertx_index_search_filtered.argtypes = [vp, vp, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]
        L.bertx_index_search_filtered_device.restype = c_i32
        L.bertx_index_search_filtered_device.argtypes = [vp, vp, c_i32, c_i32, vp, c_i32, c_i32, vp, vp, vp]
        L.bertx_index_search_rescored_filtered.restype = c_i32
        L.bertx_index_search_rescored_filtered.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]
        L.bertx_index_search_rescored_filtered_device.restype = c_i32
        L.bertx_index_search_rescored_filtered_device.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp,
                                                                  vp]
        L.bertx_index_search_rescored_texts.restype = c_i32
        L.bertx_index_search_rescored_texts.argtypes = [vp, vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32,
                                                        c_i32, vp, vp]
        L.bertx_bench_search_rescored.restype = c_i32
        L.bertx_bench_search_rescored.argtypes = [c_i32] * 7 + [c_f32p]
    except AttributeError:
        pass
    try:   # (cross-encoder reranking: absent from older BERT_LIB builds)
        L.bertx_convert_hf_head.restype = c_i32
        L.bertx_convert_hf_head.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_i32]
        L.bertx_n_labels.restype = c_i32
        L.bertx_n_labels.argtypes = [vp]
        L.bertx_tokenize_pair.restype = c_i32
        L.bertx_tokenize_pair.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, c_i32, vp, vp, c_i32p, c_i32]
        L.bertx_forward_device_ex.restype = c_i32
        L.bertx_forward_device_ex.argtypes = [vp, c_i32, vp, vp, vp, c_i32, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_score_ids.restype = c_i32
        L.bertx_score_ids.argtypes = [vp, c_i32, vp, vp, vp, vp]
        L.bertx_score_pairs.restype = c_i32
        L.bertx_score_pairs.argtypes = [vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p),
                                        ctypes.POINTER(ctypes.c_char_p), c_i32, vp]
        L.bertx_rerank.restype = c_i32
        L.bertx_rerank.argtypes = [vp, c_i32, ctypes.c_char_p, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32, vp]
        L.bertx_test_head.restype = c_i32
        L.bertx_test_head.argtypes = [vp, c_i32, c_i32, vp, vp, vp, vp, c_i32, vp, c_i32]
        L.bertx_test_embed_ln_types.restype = c_i32
        L.bertx_test_embed_ln_types.argtypes = [c_i32] * 7 + [vp] * 8 + [c_i32, c_i32, vp, vp, c_i32]
    except AttributeError:
        pass
    try:   # (the token store of late interaction: absent from older BERT_LIB builds)
        c_i64 = ctypes.c_int64
        L.bertx_mvindex_create.restype = vp
        L.bertx_mvindex_create.argtypes = [vp, c_i32, c_i32, c_i32, c_i64]
        L.bertx_mvindex_create_ex.restype = vp
        L.bertx_mvindex_create_ex.argtypes = [vp, c_i32, c_i32, c_i32, c_i64, c_i32]
        L.bertx_mvindex_storage.restype = c_i32
        L.bertx_mvindex_storage.argtypes = [vp]
        L.bertx_mvindex_doc_i8.restype = c_i32
        L.bertx_mvindex_doc_i8.argtypes = [vp, c_i32, vp, vp]
        L.bertx_bench_maxsim_ex.restype = c_i32
        L.bertx_bench_maxsim_ex.argtypes = [c_i32] * 7 + [c_f32p]
        L.bertx_mvindex_free.restype = None
        L.bertx_mvindex_free.argtypes = [vp]
        for fn in (L.bertx_mvindex_clear, L.bertx_mvindex_docs, L.bertx_mvindex_capacity_docs, L.bertx_mvindex_dim):
            fn.restype = c_i32
            fn.argtypes = [vp]
        for fn in (L.bertx_mvindex_token_slots, L.bertx_mvindex_capacity_token_slots):
            fn.restype = c_i64
            fn.argtypes = [vp]
        L.bertx_mvindex_add.restype = c_i32
        L.bertx_mvindex_add.argtypes = [vp, vp, vp, c_i32]
        L.bertx_mvindex_add_device.restype = c_i32
        L.bertx_mvindex_add_device.argtypes = [vp, vp, vp, c_i32, vp]
        L.bertx_mvindex_doc_len.restype = c_i32
        L.bertx_mvindex_doc_len.argtypes = [vp, c_i32]
        L.bertx_mvindex_doc.restype = c_i32
        L.bertx_mvindex_doc.argtypes = [vp, c_i32, vp]
        L.bertx_mvindex_score.restype = c_i32
        L.bertx_mvindex_score.argtypes = [vp, vp, c_i32, vp, c_i32, vp]
        L.bertx_mvindex_score_device.restype = c_i32
        L.bertx_mvindex_score_device.argtypes = [vp, vp, c_i32, vp, c_i32, vp, vp]
        L.bertx_mvindex_add_texts.restype = c_i32
        L.bertx_mvindex_add_texts.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p)]
        L.bertx_mvindex_score_text.restype = c_i32
        L.bertx_mvindex_score_text.argtypes = [vp, vp, ctypes.c_char_p, vp, c_i32, vp]
        L.bertx_bench_maxsim.restype = c_i32
        L.bertx_bench_maxsim.argtypes = [c_i32] * 6 + [c_f32p]
        L.bertx_mvindex_search.restype = c_i32
        L.bertx_mvindex_search.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_search_device.restype = c_i32
        L.bertx_mvindex_search_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, vp, vp]
        L.bertx_mvindex_search_texts.restype = c_i32
        L.bertx_mvindex_search_texts.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32, vp, vp]
        L.bertx_mvindex_search_texts_colbert.restype = c_i32
        L.bertx_mvindex_search_texts_colbert.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32,
                                                         c_i32, vp, vp]
        L.bertx_bench_maxsim_search.restype = c_i32
        L.bertx_bench_maxsim_search.argtypes = [c_i32] * 8 + [c_f32p]
    except AttributeError:
        pass
    try:   # (centroid codes and the pruned search of the token store: absent from older BERT_LIB builds)
        c_i64 = ctypes.c_int64
        c_u32 = ctypes.c_uint32
        L.bertx_mvindex_set_centroids.restype = c_i32
        L.bertx_mvindex_set_centroids.argtypes = [vp, vp, c_i32]
        L.bertx_mvindex_train_centroids.restype = c_i32
        L.bertx_mvindex_train_centroids.argtypes = [vp, c_i32, c_i32, c_u32]
        L.bertx_mvindex_centroids.restype = c_i32
        L.bertx_mvindex_centroids.argtypes = [vp]
        L.bertx_mvindex_centroid.restype = c_i32
        L.bertx_mvindex_centroid.argtypes = [vp, c_i32, vp]
        L.bertx_mvindex_doc_codes.restype = c_i32
        L.bertx_mvindex_doc_codes.argtypes = [vp, c_i32, vp]
        L.bertx_mvindex_candidates.restype = c_i32
        L.bertx_mvindex_candidates.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_candidates_device.restype = c_i32
        L.bertx_mvindex_candidates_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, vp, vp]
        L.bertx_mvindex_search_pruned.restype = c_i32
        L.bertx_mvindex_search_pruned.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_search_pruned_device.restype = c_i32
        L.bertx_mvindex_search_pruned_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp, vp, vp]
        L.bertx_mvindex_search_pruned_texts.restype = c_i32
        L.bertx_mvindex_search_pruned_texts.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32, c_i32,
                                                        c_i32, vp, vp]
        L.bertx_bench_maxsim_pruned.restype = c_i32
        L.bertx_bench_maxsim_pruned.argtypes = [c_i32] * 10 + [c_f32p]
        L.bertx_test_approx_ran.restype = c_i32
        L.bertx_test_approx_ran.argtypes = [c_i32]
        L.bertx_test_kmeans_update.restype = c_i32
        L.bertx_test_kmeans_update.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp]
        L.bertx_test_kmeans_sample.restype = c_i32
        L.bertx_test_kmeans_sample.argtypes = [c_i64, c_u32, vp]
    except AttributeError:
        pass
    try:   # (the cap on a token store's scan grids, a test hook; absent from older BERT_LIB builds)
        L.bertx_test_mvindex_grid.restype = c_i32
        L.bertx_test_mvindex_grid.argtypes = [vp, c_i32]
        L.bertx_test_mvindex_last_grid.restype = c_i32
        L.bertx_test_mvindex_last_grid.argtypes = [vp]
    except AttributeError:
        pass
    try:   # (document deletion and filtered search of the token store; absent from older BERT_LIB builds)
        L.bertx_mvindex_remove.restype = c_i32
        L.bertx_mvindex_remove.argtypes = [vp, vp, c_i32]
        L.bertx_mvindex_remove_device.restype = c_i32
        L.bertx_mvindex_remove_device.argtypes = [vp, vp, c_i32, vp]
        L.bertx_mvindex_live.restype = c_i32
        L.bertx_mvindex_live.argtypes = [vp]
        L.bertx_mvindex_deleted.restype = c_i32
        L.bertx_mvindex_deleted.argtypes = [vp, c_i32, c_i32, vp]
        L.bertx_mvindex_search_filtered.restype = c_i32
        L.bertx_mvindex_search_filtered.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_search_filtered_device.restype = c_i32
        L.bertx_mvindex_search_filtered_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp, vp]
        L.bertx_mvindex_candidates_filtered.restype = c_i32
        L.bertx_mvindex_candidates_filtered.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_candidates_filtered_device.restype = c_i32
        L.bertx_mvindex_candidates_filtered_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp, vp]
        L.bertx_mvindex_search_pruned_filtered.restype = c_i32
        L.bertx_mvindex_search_pruned_filtered.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp]
        L.bertx_mvindex_search_pruned_filtered_device.restype = c_i32
        L.bertx_mvindex_search_pruned_filtered_device.argtypes = [vp, vp, c_i32, c_i32, c_i32, c_i32, vp, c_i32, c_i32, vp, vp,
                                                                  vp]
        L.bertx_test_mvindex_last_masked.restype = c_i32
        L.bertx_test_mvindex_last_masked.argtypes = [vp]
        L.bertx_bench_maxsim_masked.restype = c_i32
        L.bertx_bench_maxsim_masked.argtypes = [c_i32] * 11 + [c_f32p]
    except AttributeError:
        pass
    try:   # (residual-coded token stores; absent from older BERT_LIB builds)
        L.bertx_mvindex_set_residual_buckets.restype = c_i32
        L.bertx_mvindex_set_residual_buckets.argtypes = [vp, vp, vp]
        L.bertx_mvindex_train_residual_buckets.restype = c_i32
        L.bertx_mvindex_train_residual_buckets.argtypes = [vp, c_i32, vp, vp]
        L.bertx_mvindex_doc_residual.restype = c_i32
        L.bertx_mvindex_doc_residual.argtypes = [vp, c_i32, vp, vp, vp]
        L.bertx_bench_maxsim_res.restype = c_i32
        L.bertx_bench_maxsim_res.argtypes = [c_i32] * 8 + [c_f32p]
    except AttributeError:
        pass
    try:   # (ColBERT checkpoints: the projection record and its entries; absent from older BERT_LIB builds)
        L.bertx_convert_hf_colbert.restype = c_i32
        L.bertx_convert_hf_colbert.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_i32]
        for fn in (L.bertx_proj_dim, L.bertx_proj_width):
            fn.restype = c_i32
            fn.argtypes = [vp]
        L.bertx_tokenize_colbert.restype = c_i32
        L.bertx_tokenize_colbert.argtypes = [vp, ctypes.c_char_p, c_i32, c_i32, vp, vp, c_i32p]
        L.bertx_forward_project_device.restype = c_i32
        L.bertx_forward_project_device.argtypes = [vp, c_i32, vp, vp, vp, c_i32, c_i32, c_i32, vp, c_i32, vp, vp]
        L.bertx_forward_project.restype = c_i32
        L.bertx_forward_project.argtypes = [vp, c_i32, ctypes.POINTER(c_i32p), c_i32p, ctypes.POINTER(c_f32p)]
        L.bertx_mvindex_add_texts_colbert.restype = c_i32
        L.bertx_mvindex_add_texts_colbert.argtypes = [vp, vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32]
        L.bertx_mvindex_score_text_colbert.restype = c_i32
        L.bertx_mvindex_score_text_colbert.argtypes = [vp, vp, ctypes.c_char_p, c_i32, vp, c_i32, vp]
        L.bertx_test_project.restype = c_i32
        L.bertx_test_project.argtypes = [c_i32, vp, vp, vp, vp, c_i32, c_i32, vp, c_i32, vp, c_i32, vp, c_i32]
        L.bertx_bench_project.restype = c_i32
        L.bertx_bench_project.argtypes = [c_i32] * 4 + [c_f32p]
    except AttributeError:
        pass
    try:   # (key counts: [MASK] rows that are not attention keys; absent from older BERT_LIB builds)
        L.bertx_forward_device_kv.restype = c_i32
        L.bertx_forward_device_kv.argtypes = [vp, c_i32, vp, vp, vp, vp, c_i32, c_i32, c_i32, c_i32, vp, c_i32, vp, vp]
        for fn in (L.bertx_forward_tokens_kv, L.bertx_forward_project_kv):
            fn.restype = c_i32
            fn.argtypes = [vp, c_i32, ctypes.POINTER(c_i32p), c_i32p, c_i32p, ctypes.POINTER(c_f32p)]
        L.bertx_tokenize_colbert_ex.restype = c_i32
        L.bertx_tokenize_colbert_ex.argtypes = [vp, ctypes.c_char_p, c_i32, c_i32, vp, vp, c_i32p, c_i32p]
        L.bertx_set_mask_keys.restype = c_i32
        L.bertx_set_mask_keys.argtypes = [vp, c_i32]
        L.bertx_mask_keys.restype = c_i32
        L.bertx_mask_keys.argtypes = [vp]
        L.bertx_test_attention_kv.restype = c_i32
        L.bertx_test_attention_kv.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, c_i32, vp]
        L.bertx_test_attention_f32_kv.restype = c_i32
        L.bertx_test_attention_f32_kv.argtypes = [vp, vp, vp, c_i32, c_i32, c_i32, c_i32, c_i32, vp, c_i32]
        L.bertx_bench_attention_kv.restype = c_i32
        L.bertx_bench_attention_kv.argtypes = [c_i32] * 7 + [c_f32p]
    except AttributeError:
        pass
    L.bertx_bench_gemm.restype = c_i32
    L.bertx_bench_gemm.argtypes = [c_i32] * 7 + [c_f32p]
    L.bertx_bench_attention.restype = c_i32
    L.bertx_bench_attention.argtypes = [c_i32] * 6 + [c_f32p]
    L.bertx_tokenize_batch.restype = c_i32
    L.bertx_tokenize_batch.argtypes = [vp, c_i32, c_i32, ctypes.POINTER(ctypes.c_char_p), c_i32, vp, vp]
    L.bertx_version.restype = ctypes.c_char_p
    L.ggml_time_us.restype = ctypes.c_int64
    if path is None:
        _lib = L
    return L


def _as_i32p(a):
    return a.ctypes.data_as(c_i32p)


def _as_f32p(a):
    return a.ctypes.data_as(c_f32p)


class BertModel:
    """Same surface as the reference client's BertModel (examples/sample_dylib.py:17-62)."""

    N_THREADS = 6   # sample_dylib.py:7

    ACT_MODES = {"f16": 0, "q8": 1}

    def __init__(self, fname, lib=None, act=None):
        """act: None = the plain ABI call (the mode comes from BERT_ACT, default f16);
        "f16" / "q8" = bertx_load_from_file with that activation mode ("q8": the
        reference's q8-activation arithmetic, quantized files only)."""
        self.lib = lib or load_lib()
        if act is None:
            self.ctx = self.lib.bert_load_from_file(fname.encode("utf-8"))
        else:
            if act not in self.ACT_MODES:
                raise ValueError("act must be None, 'f16' or 'q8', not %r" % (act,))
            self.ctx = self.lib.bertx_load_from_file(fname.encode("utf-8"), self.ACT_MODES[act])
        if not self.ctx:
            raise RuntimeError("bert_load_from_file failed for " + fname)
        self.n_embd = self.lib.bert_n_embd(self.ctx)
        self.n_max_tokens = self.lib.bert_n_max_tokens(self.ctx)

    def __del__(self):
        if getattr(self, "ctx", None):
            self.lib.bert_free(self.ctx)
            self.ctx = None

    @property
    def activation_mode(self):
        """The activation mode the context runs: 0 = f16, 1 = the reference's q8."""
        return int(self.lib.bertx_activation_mode(self.ctx))

    POOL_MODES = {"mean": 0, "cls": 1}

    @property
    def pooling(self):
        """The pooling mode of the sentence embeddings: "mean" (default) or "cls"."""
        v = int(self.lib.bertx_pooling(self.ctx))
        return next(k for k, x in self.POOL_MODES.items() if x == v)

    def set_pooling(self, mode):
        """"mean": masked mean of the final rows; "cls": the first token's row; both L2-normalised."""
        if mode not in self.POOL_MODES:
            raise ValueError("pooling must be 'mean' or 'cls', not %r" % (mode,))
        if self.lib.bertx_set_pooling(self.ctx, self.POOL_MODES[mode]) != 0:
            raise RuntimeError("bertx_set_pooling failed")

    def set_cls_pruning(self, on):
        """Whether CLS pooling runs the last layer on the sentences' first rows only (default on)."""
        self.lib.bertx_set_cls_pruning(self.ctx, 1 if on else 0)

    @property
    def mask_keys(self):
        """Whether the store's ColBERT query forms keep the [MASK] rows as attention keys (default True)."""
        return bool(self.lib.bertx_mask_keys(self.ctx))

    def set_mask_keys(self, on):
        """False: score_text / search_texts with colbert= let no row attend to a query's [MASK] rows
        (ColBERT's attend_to_mask_tokens = false); True: the [MASK] rows are ordinary keys."""
        if self.lib.bertx_set_mask_keys(self.ctx, 1 if on else 0) != 0:
            raise RuntimeError("bertx_set_mask_keys failed")

    def _forward_rows(self, fn, name, ids_list, width, n_keys=None):
        n = len(ids_list)
        lens = np.fromiter((len(x) for x in ids_list), np.int32, n)
        flat = (np.concatenate(ids_list) if n else np.zeros(0)).astype(np.int32, copy=False)
        flat = np.ascontiguousarray(flat)
        out = np.zeros((int(lens.sum()), width), np.float32)
        offs = np.zeros(n, np.uintp)
        if n > 1:
            np.cumsum(lens[:-1], out=offs[1:])
        tp = (flat.ctypes.data + 4 * offs).astype(np.uintp)
        op = (out.ctypes.data + out.strides[0] * offs).astype(np.uintp)
        if n_keys is None:
            rc = fn(self.ctx, n, tp.ctypes.data_as(ctypes.POINTER(c_i32p)), _as_i32p(lens),
                    op.ctypes.data_as(ctypes.POINTER(c_f32p)))
        else:
            keys = np.ascontiguousarray(n_keys, np.int32)
            if keys.shape != (n,):
                raise ValueError("n_keys must hold one count per sentence")
            rc = fn(self.ctx, n, tp.ctypes.data_as(ctypes.POINTER(c_i32p)), _as_i32p(lens), _as_i32p(keys),
                    op.ctypes.data_as(ctypes.POINTER(c_f32p)))
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (name, rc))
        return [out[int(o):int(o) + int(l)] for o, l in zip(offs, lens)]

    def forward_tokens(self, ids_list, n_keys=None):
        """Per-token final hidden states (un-normalised): a list of [len][n_embd] f32 arrays.
        n_keys: one count per sentence, 1 .. its length: only its first n_keys[i] rows are
        attention keys (every row is still a query and an output row)."""
        if n_keys is not None:
            return self._forward_rows(self.lib.bertx_forward_tokens_kv, "bertx_forward_tokens_kv", ids_list, self.n_embd,
                                      n_keys)
        return self._forward_rows(self.lib.bertx_forward_tokens, "bertx_forward_tokens", ids_list, self.n_embd)

    # -- ColBERT checkpoints: files with a linear.weight record --
    @property
    def proj_dim(self):
        """Rows of the file's ColBERT projection, 0 for a file without one."""
        return int(self.lib.bertx_proj_dim(self.ctx))

    @property
    def proj_width(self):
        """Width of every projected row, 64 ceil(proj_dim / 64): a legal BertTokenIndex width."""
        return int(self.lib.bertx_proj_width(self.ctx))

    def tokenize_colbert(self, text, kind, maxlen, with_keys=False):
        """(ids, keep) of a query ("query" / 0: [CLS] [Q] pieces [SEP] and [MASK] up to maxlen) or a
        document ("doc" / 1: [CLS] [D] pieces [SEP], keep 0 on punctuation tokens).  with_keys:
        (ids, keep, n_keys), the count of rows up to and including [SEP] for a query, all for a document."""
        kind = {"query": 0, "doc": 1}.get(kind, kind)
        ids, keep, n = np.zeros(max(maxlen, 1), np.int32), np.zeros(max(maxlen, 1), np.int32), c_i32(0)
        if with_keys:
            nk = c_i32(0)
            rc = self.lib.bertx_tokenize_colbert_ex(self.ctx, self._bytes(text), kind, maxlen, ids.ctypes.data,
                                                    keep.ctypes.data, ctypes.byref(n), ctypes.byref(nk))
            if rc != 0:
                raise ValueError("bertx_tokenize_colbert_ex failed (%d)" % rc)
            return ids[:n.value].copy(), keep[:n.value].copy(), int(nk.value)
        rc = self.lib.bertx_tokenize_colbert(self.ctx, self._bytes(text), kind, maxlen, ids.ctypes.data, keep.ctypes.data,
                                             ctypes.byref(n))
        if rc != 0:
            raise ValueError("bertx_tokenize_colbert failed (%d)" % rc)
        return ids[:n.value].copy(), keep[:n.value].copy()

    def forward_project(self, ids_list, n_keys=None):
        """Per-token unit-length projected rows: a list of [len][proj_width] f32 arrays; n_keys as forward_tokens."""
        if n_keys is not None:
            return self._forward_rows(self.lib.bertx_forward_project_kv, "bertx_forward_project_kv", ids_list,
                                      self.proj_width, n_keys)
        return self._forward_rows(self.lib.bertx_forward_project, "bertx_forward_project", ids_list, self.proj_width)

    def encode(self, sentences, batch_size=16):
        input_is_string = isinstance(sentences, str)
        if input_is_string:
            sentences = [sentences]
        n = len(sentences)
        embeddings = np.zeros((n, self.n_embd), dtype=np.float32)
        ptrs = (embeddings.ctypes.data + embeddings.strides[0] * np.arange(n, dtype=np.uintp)).astype(np.uintp)
        ptrs = ptrs.ctypes.data_as(ctypes.POINTER(c_f32p))
        texts = (ctypes.c_char_p * n)()
        for j, s in enumerate(sentences):
            texts[j] = s.encode("utf-8") if isinstance(s, str) else s
        self.lib.bert_encode_batch(self.ctx, self.N_THREADS, batch_size, n, texts, ptrs)
        return embeddings[0] if input_is_string else embeddings

    # -- separate tokenization / forward (bert.h:56-85) --
    def tokenize(self, text, n_max_tokens=None):
        if isinstance(text, str):
            text = text.encode("utf-8")
        n_max = self.n_max_tokens if n_max_tokens is None else n_max_tokens
        buf = np.zeros(max(n_max, 1), np.int32)
        n = c_i32(0)
        self.lib.bert_tokenize(self.ctx, text, _as_i32p(buf), ctypes.byref(n), n_max)
        return [int(x) for x in buf[: min(n.value, n_max)]], n.value

    def id_to_token(self, i):
        return self.lib.bert_vocab_id_to_token(self.ctx, i)

    def forward_batch(self, ids_list, fake=False, fill=0.0):
        n = len(ids_list)
        lens = np.fromiter((len(x) for x in ids_list), np.int32, n)
        flat = (np.concatenate(ids_list) if n else np.zeros(0)).astype(np.int32, copy=False)
        flat = np.ascontiguousarray(flat)
        out = np.full((n, self.n_embd), fill, np.float32)
        # the int32_t* / float* arrays as address vectors into one id buffer and the
        # output rows (a ctypes pointer object per row costs ~6 us: 0.4 ms for a
        # 64-sentence batch, 5% of the forward)
        offs = np.zeros(n, np.uintp)
        if n > 1:
            np.cumsum(lens[:-1], out=offs[1:])
        tp = (flat.ctypes.data + 4 * offs).astype(np.uintp)
        op = (out.ctypes.data + out.strides[0] * np.arange(n, dtype=np.uintp)).astype(np.uintp)
        fn = self.lib.bert_forward_fake_batch if fake else self.lib.bert_forward_batch
        fn(self.ctx, self.N_THREADS, n, tp.ctypes.data_as(ctypes.POINTER(c_i32p)), _as_i32p(lens),
           op.ctypes.data_as(ctypes.POINTER(c_f32p)))
        return out

    def forward(self, ids):
        a = np.ascontiguousarray(np.asarray(ids, np.int32))
        out = np.zeros(self.n_embd, np.float32)
        self.lib.bert_forward(self.ctx, self.N_THREADS, _as_i32p(a), len(a), _as_f32p(out))
        return out

    # -- cross-encoder reranking (bert_hip.h) --
    OUT_POOLED, OUT_TOKENS, OUT_LOGITS = 0, 1, 2

    @property
    def n_labels(self):
        """Logits per pair of the file's classification head; 0: the file has none."""
        return int(self.lib.bertx_n_labels(self.ctx))

    @staticmethod
    def _bytes(s):
        return s.encode("utf-8") if isinstance(s, str) else s

    def tokenize_pair(self, a, b, truncate=True, n_max=None):
        """(ids, types) of [CLS] a [SEP] b [SEP]; a pair over n_max without `truncate` raises
        ValueError carrying the full token count."""
        n_max = self.n_max_tokens if n_max is None else n_max
        ids, types = np.zeros(max(n_max, 1), np.int32), np.zeros(max(n_max, 1), np.int32)
        n = c_i32(0)
        rc = self.lib.bertx_tokenize_pair(self.ctx, self._bytes(a), self._bytes(b), 1 if truncate else 0,
                                          ids.ctypes.data, types.ctypes.data, ctypes.byref(n), n_max)
        if rc == -4:
            raise ValueError("pair of %d tokens, maximum is %d" % (n.value, n_max))
        if rc != 0:
            raise RuntimeError("bertx_tokenize_pair failed (%d)" % rc)
        return ids[:n.value].copy(), types[:n.value].copy()

    def score_ids(self, ids_list, types_list, fill=0.0):
        """Raw logits f32 [n][n_labels] of pre-tokenised pairs."""
        n = len(ids_list)
        lens = np.fromiter((len(x) for x in ids_list), np.int32, n)
        ids = [np.ascontiguousarray(np.asarray(x, np.int32)) for x in ids_list]
        types = [np.ascontiguousarray(np.asarray(x, np.int32)) for x in types_list]
        ip = np.array([x.ctypes.data for x in ids], np.uintp)
        tp = np.array([x.ctypes.data for x in types], np.uintp)
        out = np.full((n, max(self.n_labels, 1)), fill, np.float32)
        rc = self.lib.bertx_score_ids(self.ctx, n, ip.ctypes.data, tp.ctypes.data, lens.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_score_ids failed (%d)" % rc)
        return out

    def score_pairs(self, pairs, truncate=True):
        """Raw logits f32 [n][n_labels] of (a, b) text pairs (no sigmoid / softmax applied)."""
        n = len(pairs)
        ta, tb = (ctypes.c_char_p * n)(), (ctypes.c_char_p * n)()
        for j, (a, b) in enumerate(pairs):
            ta[j], tb[j] = self._bytes(a), self._bytes(b)
        out = np.zeros((n, max(self.n_labels, 1)), np.float32)
        rc = self.lib.bertx_score_pairs(self.ctx, self.N_THREADS, n, ta, tb, 1 if truncate else 0, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_score_pairs failed (%d)" % rc)
        return out

    def rerank_logits(self, query, docs, truncate=True):
        """bertx_rerank: logits f32 [n_docs][n_labels] of (query, doc) pairs."""
        n = len(docs)
        td = (ctypes.c_char_p * n)()
        for j, s in enumerate(docs):
            td[j] = self._bytes(s)
        out = np.zeros((n, max(self.n_labels, 1)), np.float32)
        rc = self.lib.bertx_rerank(self.ctx, self.N_THREADS, self._bytes(query), n, td, 1 if truncate else 0,
                                   out.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_rerank failed (%d)" % rc)
        return out

    def rerank(self, query, docs, top_k=None):
        """[(index, logit)] of docs by descending first-label logit (equal logits by index), the best top_k."""
        lg = self.rerank_logits(query, docs)[:, 0]
        order = np.argsort(-lg, kind="stable")
        return [(int(i), float(lg[i])) for i in order[:top_k]]

    def forward_device_ex(self, slot, d_ids, d_types, d_cu, n_seqs, max_len, total_tokens, out_kind, d_out, stream):
        """bertx_forward_device_ex on raw device addresses (ints; d_types 0 / None: all type 0)."""
        return int(self.lib.bertx_forward_device_ex(self.ctx, slot, d_ids, d_types or None, d_cu, n_seqs, max_len,
                                                    total_tokens, out_kind, d_out, stream or None))

    def device_last_call(self):
        """Per GPU of the context: (wall ms, sentences, tokens) of the last host-driven call."""
        out = []
        for i in range(self.lib.bertx_num_devices(self.ctx)):
            ms, ns, nt = ctypes.c_double(), c_i32(), ctypes.c_int64()
            self.lib.bertx_device_last_call(self.ctx, i, ctypes.byref(ms), ctypes.byref(ns), ctypes.byref(nt))
            out.append((ms.value, ns.value, nt.value))
        return out

    def hparams(self):
        hp = (c_i32 * 7)()
        self.lib.bertx_hparams(self.ctx, hp)
        return list(hp)

    def kernel_stats(self):
        out = []
        i = 0
        while True:
            name = ctypes.c_char_p()
            launches = ctypes.c_int64()
            ms = ctypes.c_double()
            work = ctypes.c_double()
            flops = c_i32()
            if self.lib.bertx_kernel_stats(self.ctx, i, ctypes.byref(name), ctypes.byref(launches),
                                           ctypes.byref(ms), ctypes.byref(work), ctypes.byref(flops)) != 0:
                break
            out.append({"name": name.value.decode(), "launches": launches.value, "ms": ms.value,
                        "work": work.value, "work_is_flops": bool(flops.value)})
            i += 1
        return out


def pack_allow(allow, B, size):
    """(words uint32 [n_filters][words] or None, n_filters, words) of an allow= filter over `size`
    units (rows of a BertIndex, documents of a BertTokenIndex) for B queries: a bool / 0-1 array
    [size] (one filter for every query) or [B][size] (one per query), packed 32 units to a word,
    unit r = bit r % 32 of word r / 32, padded to whole words; or the packed words themselves, a
    uint32 array [words] or [B][words] with words >= ceil(size / 32), passed on as they are."""
    if allow is None:
        return None, 0, 0
    raw = np.asarray(allow)
    need = (size + 31) // 32
    if raw.dtype == np.uint32 and raw.shape not in ((size,), (B, size)) and raw.ndim in (1, 2) and raw.shape[-1] >= need \
            and (raw.ndim == 1 or raw.shape[0] in (1, B)):
        packed = np.ascontiguousarray(np.atleast_2d(raw))
        return packed, packed.shape[0], packed.shape[1]
    a = raw.astype(bool)
    if a.shape not in ((size,), (B, size)):
        raise ValueError("expected allow of shape (%d,) or (%d, %d), got %r" % (size, B, size, a.shape))
    a = np.atleast_2d(a)
    padded = np.zeros((a.shape[0], 32 * need), bool)
    padded[:, :size] = a
    packed = np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint32)
    return packed.reshape(a.shape[0], need), a.shape[0], need


class BertIndex:
    """A device-resident embedding index with fused top-k search (bertx_index_*): rows of
    the model's n_embd, stored as f16 (storage="f16") or as int8 with one f32 scale per
    row (storage="int8", half the bytes) on GPU `slot` of the model's context; ids are
    the insertion order.  Scores are dot products (cosines, for the model's unit rows);
    bert_hip.h gives the arithmetic of both kinds."""

    STORAGE = {"f16": 0, "int8": 1}

    def __init__(self, model, capacity, slot=0, storage="f16"):
        if storage not in self.STORAGE:
            raise ValueError("storage must be %s, got %r" % (" or ".join(repr(s) for s in self.STORAGE), storage))
        self.model = model
        self.lib = model.lib
        self.storage = storage
        self.idx = self.lib.bertx_index_create_ex(model.ctx, slot, capacity, self.STORAGE[storage])
        if not self.idx:
            raise RuntimeError("bertx_index_create_ex failed")
        self.dim = int(self.lib.bertx_index_dim(self.idx))
        self.capacity = int(self.lib.bertx_index_capacity(self.idx))

    def __del__(self):
        if getattr(self, "idx", None):
            self.lib.bertx_index_free(self.idx)
            self.idx = None

    def __len__(self):
        return int(self.lib.bertx_index_size(self.idx))

    def clear(self):
        self.lib.bertx_index_clear(self.idx)

    def _rows(self, a):
        a = np.ascontiguousarray(np.asarray(a, np.float32))
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError("expected rows of width %d, got shape %r" % (self.dim, a.shape))
        return a

    @staticmethod
    def _texts(texts):
        arr = (ctypes.c_char_p * len(texts))()
        for j, s in enumerate(texts):
            arr[j] = s.encode("utf-8") if isinstance(s, str) else s
        return arr

    def add(self, rows):
        """Append f32 rows [n][dim]; returns the id of the first one."""
        a = self._rows(rows)
        rc = self.lib.bertx_index_add(self.idx, a.ctypes.data, a.shape[0])
        if rc < 0:
            raise RuntimeError("bertx_index_add failed (%d)" % rc)
        return rc

    def add_texts(self, texts):
        """Encode (the model's pooling mode) and append; returns the id of the first new row."""
        rc = self.lib.bertx_index_add_texts(self.idx, self.model.ctx, self.model.N_THREADS, len(texts),
                                            self._texts(texts))
        if rc < 0:
            raise RuntimeError("bertx_index_add_texts failed (%d)" % rc)
        return rc

    def remove(self, ids):
        """Delete the listed rows: they are never returned again, their ids are not reused and
        len() does not change.  Ids outside the index are ignored, repeats are harmless."""
        a = np.ascontiguousarray(np.asarray(ids, np.int32).ravel())
        rc = self.lib.bertx_index_remove(self.idx, a.ctypes.data, a.size)
        if rc != 0:
            raise RuntimeError("bertx_index_remove failed (%d)" % rc)

    def live(self):
        """len() minus the deleted rows."""
        return int(self.lib.bertx_index_live(self.idx))

    def deleted(self, first, n):
        """bool [n]: whether rows first .. first + n - 1 are deleted."""
        out = np.zeros(n, np.uint8)
        if n and self.lib.bertx_index_deleted(self.idx, first, n, out.ctypes.data) != 0:
            raise RuntimeError("bertx_index_deleted failed")
        return out.astype(bool)

    def _allow(self, allow, B):
        """pack_allow over this store's len(): shared by BertIndex (rows) and BertTokenIndex
        (documents)."""
        return pack_allow(allow, B, len(self))

    def search(self, queries, k, allow=None):
        """(scores f32 [B][k], ids i32 [B][k]) of the k best rows per query, best first.  Deleted
        rows are never returned; allow (bool [size], or [B][size] for one filter per query)
        limits the search to the rows it marks."""
        q = self._rows(queries)
        scores = np.zeros((q.shape[0], k), np.float32)
        ids = np.zeros((q.shape[0], k), np.int32)
        f, nf, words = self._allow(allow, q.shape[0])
        rc = self.lib.bertx_index_search_filtered(self.idx, q.ctypes.data, q.shape[0], k, None if f is None else f.ctypes.data,
                                                  nf, words, scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_index_search failed (%d)" % rc)
        return scores, ids

    def search_texts(self, texts, k):
        scores = np.zeros((len(texts), k), np.float32)
        ids = np.zeros((len(texts), k), np.int32)
        rc = self.lib.bertx_index_search_texts(self.idx, self.model.ctx, self.model.N_THREADS, len(texts),
                                               self._texts(texts), k, scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_index_search_texts failed (%d)" % rc)
        return scores, ids

    def rows(self, first, n):
        """The stored rows first .. first + n - 1 as f32 [n][dim]: the exact f16 values, or
        the dequantized q * scale of an int8 index."""
        out = np.zeros((n, self.dim), np.float32)
        if n and self.lib.bertx_index_rows(self.idx, first, n, out.ctypes.data) != 0:
            raise RuntimeError("bertx_index_rows failed")
        return out

    def rows_i8(self, first, n):
        """(q int8 [n][dim], scale f32 [n]): the stored bytes and scales of an int8 index."""
        q = np.zeros((n, self.dim), np.int8)
        scale = np.zeros(n, np.float32)
        if n and self.lib.bertx_index_rows_i8(self.idx, first, n, q.ctypes.data, scale.ctypes.data) != 0:
            raise RuntimeError("bertx_index_rows_i8 failed")
        return q, scale

    def score_ids(self, queries, ids):
        """scores f32 [B][n]: the score of (query b, row ids[b][j]) with the bits search() gives
        that pair, -inf for an id outside the index (a search's -1 fill included); n <= 128."""
        q = self._rows(queries)
        ids = np.ascontiguousarray(np.asarray(ids, np.int32))
        if ids.ndim == 1:
            ids = ids[None, :]
        if ids.ndim != 2 or ids.shape[0] != q.shape[0]:
            raise ValueError("expected ids of shape (%d, n), got %r" % (q.shape[0], ids.shape))
        scores = np.zeros(ids.shape, np.float32)
        rc = self.lib.bertx_index_score_ids(self.idx, q.ctypes.data, q.shape[0], ids.ctypes.data, ids.shape[1],
                                            scores.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_index_score_ids failed (%d)" % rc)
        return scores

    @staticmethod
    def _n_cand(k, n_cand):
        return min(128, 4 * k) if n_cand is None else n_cand

    def search_rescored(self, queries, k, fine, n_cand=None, allow=None):
        """The two-stage search: this index finds n_cand candidates per query (default
        min(128, 4 k)), `fine` (another BertIndex of the same width whose rows were added in
        the same order) scores them, the k best by fine's scores come back.  Bit for bit
        search(n_cand, allow) -> fine.score_ids -> the order of the results."""
        q = self._rows(queries)
        scores = np.zeros((q.shape[0], k), np.float32)
        ids = np.zeros((q.shape[0], k), np.int32)
        f, nf, words = self._allow(allow, q.shape[0])
        rc = self.lib.bertx_index_search_rescored_filtered(self.idx, fine.idx, q.ctypes.data, q.shape[0], k,
                                                           self._n_cand(k, n_cand), None if f is None else f.ctypes.data, nf,
                                                           words, scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_index_search_rescored failed (%d)" % rc)
        return scores, ids

    def search_rescored_texts(self, texts, k, fine, n_cand=None):
        scores = np.zeros((len(texts), k), np.float32)
        ids = np.zeros((len(texts), k), np.int32)
        rc = self.lib.bertx_index_search_rescored_texts(self.idx, fine.idx, self.model.ctx, self.model.N_THREADS, len(texts),
                                                        self._texts(texts), k, self._n_cand(k, n_cand), scores.ctypes.data,
                                                        ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_index_search_rescored_texts failed (%d)" % rc)
        return scores, ids


class BertBinaryIndex(BertIndex):
    """A BertIndex that keeps a row as its d sign bits (bit = x > 0), one sixteenth of f16.
    A score is d - 2 hamming(bits_query, bits_row), an exact integer: the dot product of the
    two +-1 vectors, no cosine.  Its use is as the first stage of search_rescored() in front
    of an f16 or int8 BertIndex of the same rows; bert_hip.h "Binary storage"."""

    STORAGE = {"binary": 8}

    def __init__(self, model, capacity, slot=0, storage="binary"):
        super().__init__(model, capacity, slot, storage)

    def rows_bits(self, first, n):
        """The stored bits uint8 [n][dim / 8] in np.packbits order."""
        out = np.zeros((n, self.dim // 8), np.uint8)
        if n and self.lib.bertx_index_rows_bits(self.idx, first, n, out.ctypes.data) != 0:
            raise RuntimeError("bertx_index_rows_bits failed")
        return out


class BertTokenIndex:
    """A device-resident token store with a fused MaxSim scorer (bertx_mvindex_*): late
    interaction.  Documents are [len][width] token vectors, stored as unit-length rows,
    f16 (storage="f16") or int8 with one f32 per token (storage="int8", half the bytes,
    a less precise similarity), on GPU `slot` of the model's context; ids are the
    insertion order.  A query of up to 64 token vectors scores a document as
    sum_i max_j <q_i, c_j>; bert_hip.h gives the arithmetic of both kinds.  width None:
    the model's n_embd (what the text forms need).
    storage="res2" / "res4" (bert_hip.h "Residual codes"): no rows, per token the code of
    its nearest centroid, 2 or 4 bits per element for the residual and one f32; such a store
    needs set_centroids and set_residual_buckets before its first document, has no full scan
    (search_pruned only) and cannot train centroids: train those, and the buckets
    (train_residual_buckets), on an f16 store of a sample."""

    MAX_QUERY_TOKENS = 64
    STORAGE = dict(BertIndex.STORAGE, res2=4, res4=5)
    RESIDUAL_BITS = {"res2": 2, "res4": 4}

    def __init__(self, model, capacity_docs, capacity_token_slots, slot=0, width=None, storage="f16"):
        if storage not in self.STORAGE:
            raise ValueError("storage must be 'f16', 'int8', 'res2' or 'res4', got %r" % (storage,))
        self.model = model
        self.lib = model.lib
        self.storage = storage
        self.mv = self.lib.bertx_mvindex_create_ex(model.ctx, slot, model.n_embd if width is None else width,
                                                   capacity_docs, capacity_token_slots, self.STORAGE[storage])
        if not self.mv:
            raise RuntimeError("bertx_mvindex_create_ex failed")
        self.dim = int(self.lib.bertx_mvindex_dim(self.mv))
        self.capacity_docs = int(self.lib.bertx_mvindex_capacity_docs(self.mv))
        self.capacity_token_slots = int(self.lib.bertx_mvindex_capacity_token_slots(self.mv))

    def __del__(self):
        if getattr(self, "mv", None):
            self.lib.bertx_mvindex_free(self.mv)
            self.mv = None

    def __len__(self):
        return int(self.lib.bertx_mvindex_docs(self.mv))

    @property
    def token_slots(self):
        """Token slots in use: 16 ceil(len / 16) per document."""
        return int(self.lib.bertx_mvindex_token_slots(self.mv))

    def clear(self):
        self.lib.bertx_mvindex_clear(self.mv)

    _allow = BertIndex._allow

    def remove(self, ids):
        """Delete the listed documents: they are never returned again (score() gives them -inf),
        their ids are not reused, len() and token_slots do not change and doc() still answers.
        Ids outside the store are ignored, repeats are harmless."""
        a = np.ascontiguousarray(np.asarray(ids, np.int32).ravel())
        rc = self.lib.bertx_mvindex_remove(self.mv, a.ctypes.data, a.size)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_remove failed (%d)" % rc)

    def live(self):
        """len() minus the deleted documents."""
        return int(self.lib.bertx_mvindex_live(self.mv))

    def deleted(self, first, n):
        """bool [n]: whether documents first .. first + n - 1 are deleted."""
        out = np.zeros(n, np.uint8)
        if n and self.lib.bertx_mvindex_deleted(self.mv, first, n, out.ctypes.data) != 0:
            raise RuntimeError("bertx_mvindex_deleted failed")
        return out.astype(bool)

    def _tokens(self, a):
        a = np.ascontiguousarray(np.asarray(a, np.float32))
        if a.ndim == 1:
            a = a[None, :]
        if a.ndim != 2 or a.shape[1] != self.dim:
            raise ValueError("expected token rows of width %d, got shape %r" % (self.dim, a.shape))
        return a

    @staticmethod
    def _ids(ids):
        return None if ids is None else np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))

    def add(self, docs):
        """Append documents, a list of [len][width] f32 arrays; returns the id of the first one."""
        docs = [self._tokens(d) for d in docs]
        lens = np.fromiter((len(d) for d in docs), np.int32, len(docs))
        rows = np.ascontiguousarray(np.concatenate(docs)) if docs else np.zeros((0, self.dim), np.float32)
        rc = self.lib.bertx_mvindex_add(self.mv, rows.ctypes.data, lens.ctypes.data, len(docs))
        if rc < 0:
            raise RuntimeError("bertx_mvindex_add failed (%d)" % rc)
        return rc

    def add_texts(self, texts, colbert=None):
        """One document per text: its per-token final hidden states; returns the first new id.
        colbert=doc_maxlen (a model with a projection record, a store of its proj_width): the
        projected rows of the text as a ColBERT document, punctuation rows dropped."""
        if colbert is not None:
            rc = self.lib.bertx_mvindex_add_texts_colbert(self.mv, self.model.ctx, self.model.N_THREADS, len(texts),
                                                          BertIndex._texts(texts), colbert)
        else:
            rc = self.lib.bertx_mvindex_add_texts(self.mv, self.model.ctx, self.model.N_THREADS, len(texts),
                                                  BertIndex._texts(texts))
        if rc < 0:
            raise RuntimeError("bertx_mvindex_add_texts%s failed (%d)" % ("_colbert" if colbert is not None else "", rc))
        return rc

    def doc_len(self, i):
        return int(self.lib.bertx_mvindex_doc_len(self.mv, i))

    def doc(self, i):
        """The stored rows of document i as f32 [len][width]: the exact f16 values, or the
        dequantized q * u of an int8 store."""
        n = self.doc_len(i)
        if n < 1:
            raise IndexError("no document %d" % i)
        out = np.zeros((n, self.dim), np.float32)
        if self.lib.bertx_mvindex_doc(self.mv, i, out.ctypes.data) != 0:
            raise RuntimeError("bertx_mvindex_doc failed")
        return out

    def doc_i8(self, i):
        """(q int8 [len][width], u f32 [len]): the stored bytes and scales of document i of
        an int8 store."""
        n = self.doc_len(i)
        if n < 1:
            raise IndexError("no document %d" % i)
        q = np.zeros((n, self.dim), np.int8)
        u = np.zeros(n, np.float32)
        if self.lib.bertx_mvindex_doc_i8(self.mv, i, q.ctypes.data, u.ctypes.data) != 0:
            raise RuntimeError("bertx_mvindex_doc_i8 failed")
        return q, u

    def _out(self, ids):
        n = len(self) if ids is None else len(ids)
        return n, np.zeros(n, np.float32)

    def score(self, q, ids=None):
        """MaxSim scores f32 [n] of the query tokens q [Lq][width] against the documents
        `ids` (None: every document); an id that is not a document scores -inf."""
        q, ids = self._tokens(q), self._ids(ids)
        n, out = self._out(ids)
        if n == 0:
            return out
        rc = self.lib.bertx_mvindex_score(self.mv, q.ctypes.data, q.shape[0], None if ids is None else ids.ctypes.data,
                                          n, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_score failed (%d)" % rc)
        return out

    def score_text(self, query, ids=None, colbert=None):
        """colbert=query_maxlen (at most 64): the query as a ColBERT query, [MASK]-augmented; whether its
        [MASK] rows are attention keys follows the model's mask_keys setting (BertModel.set_mask_keys)."""
        ids = self._ids(ids)
        n, out = self._out(ids)
        if n == 0:
            return out
        ip = None if ids is None else ids.ctypes.data
        if colbert is not None:
            rc = self.lib.bertx_mvindex_score_text_colbert(self.mv, self.model.ctx, BertModel._bytes(query), colbert, ip, n,
                                                           out.ctypes.data)
        else:
            rc = self.lib.bertx_mvindex_score_text(self.mv, self.model.ctx, BertModel._bytes(query), ip, n, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_score_text%s failed (%d)" % ("_colbert" if colbert is not None else "", rc))
        return out

    def search(self, queries, k, allow=None):
        """(scores f32 [B][k], ids i32 [B][k]): per query the k best documents of the whole
        store by MaxSim score, best first, equal scores by ascending id, (-inf, -1) where the
        store has fewer than k documents; the scores are the bits of score().  queries: one
        [Lq][width] array or a list of them; a ragged list is padded with zero rows to the
        longest (a zero row adds +0).  At most 64 rows per query.  Deleted documents are never
        returned; allow (pack_allow: bool [docs], [B][docs] for one filter per query, or packed
        uint32 words) limits the search to the documents it marks, with (-inf, -1) where fewer
        than k are admissible (bert_hip.h "Deleting documents and filtered search")."""
        if isinstance(queries, np.ndarray) and queries.ndim <= 2:
            queries = [queries]
        qs = [self._tokens(q) for q in queries]
        if not qs:
            raise ValueError("no queries")
        Lq = max(len(q) for q in qs)
        if Lq < 1 or Lq > self.MAX_QUERY_TOKENS:
            raise ValueError("a query has %d rows, the limits are 1 .. %d" % (Lq, self.MAX_QUERY_TOKENS))
        q = np.zeros((len(qs), Lq, self.dim), np.float32)
        for i, a in enumerate(qs):
            q[i, :len(a)] = a
        scores = np.zeros((len(qs), k), np.float32)
        ids = np.zeros((len(qs), k), np.int32)
        if allow is None:
            rc = self.lib.bertx_mvindex_search(self.mv, q.ctypes.data, len(qs), Lq, k, scores.ctypes.data, ids.ctypes.data)
        else:
            f, nf, words = self._allow(allow, len(qs))
            rc = self.lib.bertx_mvindex_search_filtered(self.mv, q.ctypes.data, len(qs), Lq, k, f.ctypes.data, nf, words,
                                                        scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_search failed (%d)" % rc)
        return scores, ids

    def _queries(self, queries):
        """One [Lq][width] array or a list of them as f32 [B][Lq][width], zero rows behind the shorter."""
        if isinstance(queries, np.ndarray) and queries.ndim <= 2:
            queries = [queries]
        qs = [self._tokens(q) for q in queries]
        if not qs:
            raise ValueError("no queries")
        Lq = max(len(q) for q in qs)
        q = np.zeros((len(qs), Lq, self.dim), np.float32)
        for i, a in enumerate(qs):
            q[i, :len(a)] = a
        return q

    def set_centroids(self, cent):
        """Centroids f32 [C][width], C a multiple of 16 in 16 .. 65,536: packed as stored rows
        are; every stored token, and every token added later, gets the code of its nearest one
        (bert_hip.h "Centroid codes").  A second call replaces them; clear() keeps them."""
        cent = self._tokens(cent)
        rc = self.lib.bertx_mvindex_set_centroids(self.mv, cent.ctypes.data, len(cent))
        if rc != 0:
            raise RuntimeError("bertx_mvindex_set_centroids failed (%d)" % rc)

    def train_centroids(self, C, iters=8, seed=0):
        """Deterministic spherical k-means over a sample of the stored rows; leaves the store coded."""
        rc = self.lib.bertx_mvindex_train_centroids(self.mv, C, iters, seed)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_train_centroids failed (%d)" % rc)

    def set_residual_buckets(self, cutoffs, weights):
        """The codec of a residual store: cutoffs f32 [2^NB - 1] (finite, non-decreasing) and
        weights f32 [2^NB] (kept as f16).  Before the first document only."""
        nb = self.RESIDUAL_BITS.get(self.storage, 0)
        cutoffs = np.ascontiguousarray(np.asarray(cutoffs, np.float32).reshape(-1))
        weights = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
        if nb and (len(cutoffs) != (1 << nb) - 1 or len(weights) != 1 << nb):
            raise ValueError("expected %d cutoffs and %d weights" % ((1 << nb) - 1, 1 << nb))
        rc = self.lib.bertx_mvindex_set_residual_buckets(self.mv, cutoffs.ctypes.data, weights.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_set_residual_buckets failed (%d)" % rc)

    def train_residual_buckets(self, nbits):
        """(cutoffs f32 [2^nbits - 1], weights f32 [2^nbits]) by ColBERTv2's quantile rule over
        the residuals of this f16 store's rows against its centroids (bert_hip.h)."""
        cutoffs = np.zeros(max((1 << nbits) - 1, 1), np.float32)
        weights = np.zeros(max(1 << nbits, 1), np.float32)
        rc = self.lib.bertx_mvindex_train_residual_buckets(self.mv, nbits, cutoffs.ctypes.data, weights.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_train_residual_buckets failed (%d)" % rc)
        return cutoffs, weights

    def doc_residual(self, i):
        """(codes uint16 [len], bits uint8 [len][width NB / 8], u f32 [len]): the stored state
        of document i of a residual store; element j of a row sits in byte j NB / 8 at bit
        NB (j mod 8 / NB)."""
        n = self.doc_len(i)
        if n < 1:
            raise IndexError("no document %d" % i)
        nb = self.RESIDUAL_BITS.get(self.storage, 2)
        codes = np.zeros(n, np.uint16)
        bits = np.zeros((n, self.dim * nb // 8), np.uint8)
        u = np.zeros(n, np.float32)
        if self.lib.bertx_mvindex_doc_residual(self.mv, i, codes.ctypes.data, bits.ctypes.data, u.ctypes.data) != 0:
            raise RuntimeError("bertx_mvindex_doc_residual failed")
        return codes, bits, u

    @property
    def n_centroids(self):
        return int(self.lib.bertx_mvindex_centroids(self.mv))

    def centroid(self, c):
        """The stored values of centroid c as f32 [width] (as doc())."""
        out = np.zeros(self.dim, np.float32)
        if self.lib.bertx_mvindex_centroid(self.mv, c, out.ctypes.data) != 0:
            raise IndexError("no centroid %d" % c)
        return out

    def doc_codes(self, i):
        """uint16 [len]: per token of document i the index of its nearest centroid."""
        n = self.doc_len(i)
        if n < 1:
            raise IndexError("no document %d" % i)
        out = np.zeros(n, np.uint16)
        if self.lib.bertx_mvindex_doc_codes(self.mv, i, out.ctypes.data) != 0:
            raise RuntimeError("bertx_mvindex_doc_codes failed (no centroids?)")
        return out

    def candidates(self, queries, n_cand, allow=None):
        """(approx f32 [B][n_cand], ids i32 [B][n_cand]): per query the n_cand best documents by
        centroid interaction, MaxSim with every stored row replaced by its centroid; best
        first, equal scores by ascending id, (-inf, -1) fill.  n_cand at most 128.  Only
        admissible documents are candidates: never a deleted one, and with allow (as in
        search()) only those it marks."""
        q = self._queries(queries)
        approx = np.zeros((len(q), n_cand), np.float32)
        ids = np.zeros((len(q), n_cand), np.int32)
        if allow is None:
            rc = self.lib.bertx_mvindex_candidates(self.mv, q.ctypes.data, q.shape[0], q.shape[1], n_cand,
                                                   approx.ctypes.data, ids.ctypes.data)
        else:
            f, nf, words = self._allow(allow, q.shape[0])
            rc = self.lib.bertx_mvindex_candidates_filtered(self.mv, q.ctypes.data, q.shape[0], q.shape[1], n_cand,
                                                            f.ctypes.data, nf, words, approx.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_candidates failed (%d)" % rc)
        return approx, ids

    def search_pruned(self, queries, k, n_cand, allow=None):
        """search() over the n_cand candidates of candidates() only: their exact scores (the
        bits of score()), the k best.  k <= n_cand <= 128; with n_cand >= len(self) the result
        is search()'s.  allow as in candidates(): with n_cand at least the number of admissible
        documents the result is search(queries, k, allow)'s."""
        q = self._queries(queries)
        scores = np.zeros((len(q), k), np.float32)
        ids = np.zeros((len(q), k), np.int32)
        if allow is None:
            rc = self.lib.bertx_mvindex_search_pruned(self.mv, q.ctypes.data, q.shape[0], q.shape[1], k, n_cand,
                                                      scores.ctypes.data, ids.ctypes.data)
        else:
            f, nf, words = self._allow(allow, q.shape[0])
            rc = self.lib.bertx_mvindex_search_pruned_filtered(self.mv, q.ctypes.data, q.shape[0], q.shape[1], k, n_cand,
                                                               f.ctypes.data, nf, words, scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_search_pruned failed (%d)" % rc)
        return scores, ids

    def search_texts(self, texts, k, colbert=None, n_cand=None):
        """search() of the texts as queries; colbert=query_maxlen as in score_text.  n_cand: the
        pruned search (search_pruned) over that many candidates per query; None: the full scan."""
        scores = np.zeros((len(texts), k), np.float32)
        ids = np.zeros((len(texts), k), np.int32)
        if n_cand is not None:
            rc = self.lib.bertx_mvindex_search_pruned_texts(self.mv, self.model.ctx, self.model.N_THREADS, len(texts),
                                                            BertIndex._texts(texts), k, n_cand, colbert or 0,
                                                            scores.ctypes.data, ids.ctypes.data)
            if rc != 0:
                raise RuntimeError("bertx_mvindex_search_pruned_texts failed (%d)" % rc)
            return scores, ids
        if colbert is not None:
            rc = self.lib.bertx_mvindex_search_texts_colbert(self.mv, self.model.ctx, self.model.N_THREADS, len(texts),
                                                             BertIndex._texts(texts), colbert, k, scores.ctypes.data,
                                                             ids.ctypes.data)
        else:
            rc = self.lib.bertx_mvindex_search_texts(self.mv, self.model.ctx, self.model.N_THREADS, len(texts),
                                                     BertIndex._texts(texts), k, scores.ctypes.data, ids.ctypes.data)
        if rc != 0:
            raise RuntimeError("bertx_mvindex_search_texts%s failed (%d)" % ("_colbert" if colbert is not None else "", rc))
        return scores, ids

    def rerank(self, query, ids, top_k=None):
        """(ids, scores) of the candidates by descending MaxSim score, equal scores by
        ascending id, the best top_k.  query: a text, or token rows [Lq][width]."""
        ids = self._ids(ids)
        sc = self.score_text(query, ids) if isinstance(query, (str, bytes)) else self.score(query, ids)
        order = np.lexsort((ids, -sc.astype(np.float64)))[:top_k]
        return ids[order], sc[order]


# ---------------------------------------------------------------------------
# model files in the reference format
# ---------------------------------------------------------------------------

HEAD_NAMES = [("pooler.dense.weight", "dd"), ("pooler.dense.bias", "d"), ("classifier.weight", "cd"),
              ("classifier.bias", "c")]


def tensor_names(n_layer, head=False):
    """Tensor names and roles in converter order (convert-to-ggml.py iterates state_dict);
    head: followed by the four records of a classification head."""
    names = [("embeddings.word_embeddings.weight", "word"), ("embeddings.position_embeddings.weight", "pos"),
             ("embeddings.token_type_embeddings.weight", "type"), ("embeddings.LayerNorm.weight", "ln_w"),
             ("embeddings.LayerNorm.bias", "ln_b")]
    for i in range(n_layer):
        p = f"encoder.layer.{i}."
        names += [(p + "attention.self.query.weight", "dd"), (p + "attention.self.query.bias", "d"),
                  (p + "attention.self.key.weight", "dd"), (p + "attention.self.key.bias", "d"),
                  (p + "attention.self.value.weight", "dd"), (p + "attention.self.value.bias", "d"),
                  (p + "attention.output.dense.weight", "dd"), (p + "attention.output.dense.bias", "d"),
                  (p + "attention.output.LayerNorm.weight", "ln_w"), (p + "attention.output.LayerNorm.bias", "ln_b"),
                  (p + "intermediate.dense.weight", "fd"), (p + "intermediate.dense.bias", "f"),
                  (p + "output.dense.weight", "df"), (p + "output.dense.bias", "d"),
                  (p + "output.LayerNorm.weight", "ln_w"), (p + "output.LayerNorm.bias", "ln_b")]
    return names + (HEAD_NAMES if head else [])


def _write_tensor(f, name, a, ftype):
    """One record.  classifier.weight: f32 in every ftype and 2-D [n_labels][d] also for one label."""
    a = np.asarray(a, np.float32)
    if name == "classifier.weight":
        a = a.reshape(-1, a.shape[-1])
    nd = a.ndim
    if ftype == 1 and name.endswith(".weight") and nd == 2 and name != "classifier.weight":
        data, lt = a.astype(np.float16), 1
    else:
        data, lt = a, 0
    nb = name.encode("utf-8")
    f.write(struct.pack("<3i", nd, len(nb), lt))
    for i in range(nd):
        f.write(struct.pack("<i", a.shape[nd - 1 - i]))
    f.write(nb)
    f.write(np.ascontiguousarray(data).tobytes())


def append_head(src, dst, tensors):
    """Copy the f32 / f16 model file src to dst followed by the four head records from tensors
    (pooler.dense.weight [d][d], pooler.dense.bias [d], classifier.weight [n_labels][d],
    classifier.bias [n_labels]); quantize the result with bertx_quantize_file for the q formats."""
    with open(src, "rb") as f:
        raw = f.read()
    ftype = struct.unpack_from("<i", raw, 4 + 6 * 4)[0]
    assert ftype in (0, 1), "append_head needs an f32 or f16 file"
    with open(dst, "wb") as f:
        f.write(raw)
        for name, _ in HEAD_NAMES:
            _write_tensor(f, name, tensors[name], ftype)
    return dst


def append_projection(src, dst, W):
    """Copy the f32 / f16 model file src to dst followed by the ColBERT projection record
    linear.weight from W [dim][n_embd] (dim % 32 == 0, 32 .. 256; no bias); quantize the result
    with bertx_quantize_file for the q formats."""
    with open(src, "rb") as f:
        raw = f.read()
    ftype = struct.unpack_from("<i", raw, 4 + 6 * 4)[0]
    assert ftype in (0, 1), "append_projection needs an f32 or f16 file"
    with open(dst, "wb") as f:
        f.write(raw)
        _write_tensor(f, "linear.weight", np.asarray(W, np.float32), ftype)
    return dst


def write_model(path, hp, vocab, tensors, ftype, head=False):
    """hp: dict n_vocab,n_max_tokens,n_embd,n_intermediate,n_head,n_layer; tensors: name -> f32 array
    (torch Linear layout [out][in]).  ftype 0 (f32) or 1 (f16): 2-D '*weight' tensors stored f16
    like convert-to-ggml.py:96-101; everything else f32.  head: the four head records follow
    (classifier.weight stays f32)."""
    assert ftype in (0, 1)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", 0x67676D6C))
        f.write(struct.pack("<7i", hp["n_vocab"], hp["n_max_tokens"], hp["n_embd"], hp["n_intermediate"],
                            hp["n_head"], hp["n_layer"], ftype))
        for w in vocab:
            b = w.encode("utf-8")
            f.write(struct.pack("<i", len(b)))
            f.write(b)
        for name, _ in tensor_names(hp["n_layer"], head):
            _write_tensor(f, name, tensors[name], ftype)


ARCHS = {
    # SURVEY.md §8 shapes (hparams as the HF configs of these checkpoints)
    "all-MiniLM-L6-v2": dict(n_vocab=30522, n_max_tokens=512, n_embd=384, n_intermediate=1536, n_head=12, n_layer=6),
    "bge-base-en-v1.5": dict(n_vocab=30522, n_max_tokens=512, n_embd=768, n_intermediate=3072, n_head=12, n_layer=12),
    "bge-large-en-v1.5": dict(n_vocab=30522, n_max_tokens=512, n_embd=1024, n_intermediate=4096, n_head=16,
                              n_layer=24),
    "bge-base-zh-v1.5": dict(n_vocab=21128, n_max_tokens=512, n_embd=768, n_intermediate=3072, n_head=12,
                             n_layer=12),
}


def synthetic_vocab(n_vocab):
    """[PAD], [unused*], [UNK]=100, [CLS]=101, [SEP]=102, [MASK], then single-token words 'w<i>'
    (so a text of k such words tokenizes to exactly k+2 ids)."""
    v = ["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    v += ["w%d" % i for i in range(n_vocab - len(v))]
    return v[:n_vocab]


def bert_like_vocab(n_vocab=30522, seed=0):
    """A synthetic WordPiece vocab of BERT's size and layout (bert-base-uncased:
    [PAD], [unused0..98], [UNK]=100, [CLS]=101, [SEP]=102, [MASK]=103, single
    characters and their '##' forms, then whole words, then '##' word pieces):
    ASCII punctuation/digits/letters, Latin-1 and Greek letters, 2-byte and 3-byte
    (CJK) characters, ~21k whole words of 2-14 letters and ~6k '##' pieces of
    1-6 letters, with a few duplicates (first-wins / last-wins map semantics,
    bert.cpp:475-494).  Deterministic in `seed`."""
    rng = np.random.default_rng(seed)
    v = ["[PAD]"] + ["[unused%d]" % i for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    chars = [chr(c) for c in range(33, 127)] + [chr(c) for c in range(0xA1, 0x180) if chr(c).isprintable()]
    chars += [chr(c) for c in range(0x391, 0x3CA)] + [chr(0x4E00 + int(i)) for i in rng.choice(20000, 600, False)]
    chars += [chr(0x3000 + i) for i in range(1, 32)]
    v += chars + ["##" + c for c in chars if c.isalnum()]
    letters = np.array(list("etaoinshrdlcumwfgypbvkjxqz"))
    freq = np.array([12.7, 9.1, 8.2, 7.5, 7.0, 6.7, 6.3, 6.1, 6.0, 4.3, 4.0, 2.8, 2.8, 2.4, 2.4, 2.2, 2.0, 2.0,
                     1.9, 1.5, 1.0, 0.8, 0.2, 0.2, 0.1, 0.1])
    freq = freq / freq.sum()
    seen = set(v)

    def word(lo, hi):
        return "".join(rng.choice(letters, int(rng.integers(lo, hi + 1)), p=freq))
    n_sub = 6000
    while len(v) < n_vocab - n_sub:
        w = word(2, 14)
        if w not in seen or rng.random() < 0.002:    # rare duplicates: token_to_id keeps the first
            seen.add(w)
            v.append(w)
    while len(v) < n_vocab:
        w = "##" + word(1, 6)
        if w not in seen or rng.random() < 0.002:    # subword_token_to_id keeps the last
            seen.add(w)
            v.append(w)
    return v[:n_vocab]


def bert_like_texts(vocab, n, n_words, seed=0):
    """Texts over a bert_like_vocab: mostly whole words, words glued from a word and
    '##' pieces (re-split by greedy longest-prefix matching), capitalised and accented
    forms, unknown letter runs, numbers, punctuation attached to words, CJK runs,
    2-4-byte characters outside the vocab, and irregular whitespace."""
    rng = np.random.default_rng(seed)
    whole = [w for w in vocab[104:] if w.isalpha() and not w.startswith("##") and len(w) > 1]
    subs = [w[2:] for w in vocab if w.startswith("##") and len(w) > 3]
    cjk = [w for w in vocab[104:] if len(w) == 1 and ord(w) >= 0x3400]
    acc = ["café", "naïve", "Über", "ÉCOLE", "résumé", "Ångström", "façade"]
    seps = [" ", " ", " ", " ", "  ", "\n", "\t", " \r\n "]
    out = []
    for _ in range(n):
        parts = []
        for _ in range(n_words):
            r = rng.random()
            if r < 0.55:
                w = whole[int(rng.integers(len(whole)))]
            elif r < 0.75:
                w = whole[int(rng.integers(len(whole)))] + "".join(
                    subs[int(rng.integers(len(subs)))] for _ in range(int(rng.integers(1, 3))))
            elif r < 0.80:
                w = whole[int(rng.integers(len(whole)))].capitalize()
            elif r < 0.83:
                w = acc[int(rng.integers(len(acc)))]
            elif r < 0.87:
                w = "".join(chr(int(c)) for c in rng.integers(97, 123, int(rng.integers(3, 16))))
            elif r < 0.90:
                w = str(int(rng.integers(0, 100000)))
            elif r < 0.95:
                w = rng.choice(["(", '"', "'"]) + whole[int(rng.integers(len(whole)))] + rng.choice([",", ".", "!", "?", ");", "'s"])
            elif r < 0.98:
                w = "".join(cjk[int(rng.integers(len(cjk)))] for _ in range(int(rng.integers(1, 5))))
            else:
                w = rng.choice(["\u00e9t\u00e9", "\U0001F600ok", "\u0416\u0437", "x\u2014y", "\uFF01", "a\u0301"])
            parts.append(str(w))
            parts.append(seps[int(rng.integers(len(seps)))])
        out.append("".join(parts).encode("utf-8"))
    return out


def outlier_channels(d, seed=1234):
    """The residual-stream channels the "sharp" profile drives to |x| ~ 50-200."""
    return np.sort(np.random.default_rng(seed + 1).choice(d, 3, replace=False))


def synthetic_tensors(hp, seed=1234, profile="survey", qk_std=None):
    """Random weights, numpy default_rng(seed).

    profile "survey" (the bench's weights): matrices and biases
    N(0, 0.02), LN gamma 1+N(0,0.02), beta N(0, 0.02).  At that scale attention
    is close to uniform, which hides key/value permutation and masking errors.

    profile "sharp" (parity tests at full size, tuned on a float64 forward so that
    rows stay distinct through every layer): LN gamma 4*(1+N(0,0.3)), Q/K matrices
    N(0, 0.05) (N(0, 0.02) past 12 layers) -- softmax rows are peaked (mean
    max-probability 0.1-0.9 per layer),
    so the attention kernel's offset/rescale path runs and a key permutation or
    mask error shows -- other matrices N(0, 0.02), embedding tables N(0, 0.5), and
    three residual outlier channels (`outlier_channels`) the way trained BERT/BGE
    checkpoints have them: O-proj and FFN-down biases of +-30/60/90 there with LN
    gains of 0.3, so the pre-LN (f16) residual stream reaches |x| ~ 100 on those
    channels while they do not swamp the LayerNorm.

    profile "sharp_mean": "sharp" plus a constant +16 on every channel of the
    O-proj and FFN-down biases, so every pre-LN residual row carries a mean of
    ~16 against a spread of a few units (the regime where the LN fold's
    z = f16(y * gamma) rounds with |y| rather than |y - mean|).

    qk_std (sharp profiles): overrides the Q/K matrices' spread (the q8-activation
    envelope sweep, scripts/q8_envelope.py)."""
    rng = np.random.default_rng(seed)
    d, f = hp["n_embd"], hp["n_intermediate"]
    shapes = {"word": (hp["n_vocab"], d), "pos": (hp["n_max_tokens"], d), "type": (2, d), "dd": (d, d),
              "fd": (f, d), "df": (d, f), "d": (d,), "f": (f,), "ln_w": (d,), "ln_b": (d,)}
    sharp = profile in ("sharp", "sharp_mean")
    assert profile in ("survey", "sharp", "sharp_mean"), profile
    oc = outlier_channels(d, seed) if sharp else None
    # Q/K spread: 24 layers of peaked attention amplify the reference's own q8
    # activation rounding (bge-large at 0.05: oracle vs the same oracle with f32
    # activations 0.88 cosine; at 0.02: >= 0.99966, the 3-token sentence worst)
    qk_std = np.float32(qk_std if qk_std is not None else 0.05 if hp["n_layer"] <= 12 else 0.02)
    out = {}
    for name, role in tensor_names(hp["n_layer"]):
        s = np.float32(0.02)
        if sharp and role in ("word", "pos", "type"):
            s = np.float32(0.5)
        if sharp and (".query." in name or ".key." in name) and role == "dd":
            s = qk_std
        a = rng.standard_normal(shapes[role], dtype=np.float32) * s
        if role == "ln_w":
            if sharp:
                a = np.float32(4.0) * (np.float32(1.0) + a * np.float32(15.0))
                a[oc] = np.float32(0.3)
            else:
                a += np.float32(1.0)
        if sharp and role == "d" and name.endswith("output.dense.bias"):
            a[oc] += np.float32([30.0, -60.0, 90.0]) * np.float32(min(1.0, d / 768))
            if profile == "sharp_mean":
                a += np.float32(16.0)
        out[name] = a
    return out


def synthetic_model(path, arch, ftype="q4_0", seed=1234, lib=None, profile="survey", qk_std=None, vocab=None):
    """Write a random-init model of `arch` in `ftype`.  Quantized files follow
    run_conversions.sh:5-8: f32 -> f16 file -> quantize from the f16 values.
    vocab: the token list (default synthetic_vocab; e.g. bert_like_vocab for
    multilingual text)."""
    hp = ARCHS[arch] if isinstance(arch, str) else arch
    vocab = synthetic_vocab(hp["n_vocab"]) if vocab is None else list(vocab)
    assert len(vocab) == hp["n_vocab"]
    tensors = synthetic_tensors(hp, seed, profile, qk_std)
    if ftype in ("f32", "f16"):
        write_model(path, hp, vocab, tensors, FTYPE[ftype])
        return path
    tmp = path + ".f16.tmp"
    write_model(tmp, hp, vocab, tensors, 1)
    L = lib or load_lib()
    rc = L.bertx_quantize_file(tmp.encode(), path.encode(), FTYPE[ftype])
    os.remove(tmp)
    if rc != 0:
        raise RuntimeError("quantize failed")
    return path


def synthetic_ids(n, length, n_vocab, seed=7):
    """Token ids per SURVEY.md §8d: uniform in [1000, V) with [CLS] first, [SEP] last."""
    rng = np.random.default_rng(seed)
    out = []
    for L in (length if hasattr(length, "__len__") else [length] * n):
        x = rng.integers(1000, n_vocab, int(L), dtype=np.int32)
        x[0], x[-1] = 101, 102
        out.append(x)
    return out
