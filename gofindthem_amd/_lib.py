"""ctypes binding of libgft.so (include/gft.h).  Fails loudly when the library is missing: there is no
Python/CPU implementation of the hot path in this package."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GFT_LIBRARY") or os.path.join(HERE, "libgft.so")   # GFT_LIBRARY: another build (tools/asan_host.sh)

GFT_OK, GFT_E_INVALID, GFT_E_NOT_BUILT, GFT_E_HIP, GFT_E_UNSUPPORTED, GFT_E_PARSE, GFT_E_ENGINE = 0, -1, -2, -3, -4, -5, -6
GFT_E_NOMEM, GFT_E_INTERNAL, GFT_W_NO_RCCL = -7, -8, 1
GFT_POS_START, GFT_POS_END = 0, 1
GFT_JSON_OK, GFT_JSON_SYNTAX, GFT_JSON_DEPTH, GFT_JSON_PATH, GFT_JSON_KEY, GFT_JSON_DUP, GFT_JSON_TEXT = range(7)
GFT_FOLD_ASCII = 1
GFT_STATS_ACCUMULATE = 1
GFT_SCORE_DISTINCT = 1
GFT_SCAN_UNIQUE = 2
GFT_POS_RUNES = 4
OP_UNIT, OP_AND, OP_OR, OP_NOT, OP_INORD = 1, 2, 3, 4, 5
INORD_FLAG = 1 << 27


class GftMatches(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("n_matches", C.c_uint64), ("match_off", C.c_void_p),
                ("term_id", C.c_void_p), ("pos", C.c_void_p)]


class GftSparse(C.Structure):
    _fields_ = [("n_docs", C.c_uint64), ("total", C.c_uint64), ("row_off", C.c_void_p), ("expr_idx", C.c_void_p),
                ("label", C.c_void_p)]


class GftExtra(C.Structure):
    _fields_ = [("off", C.c_void_p), ("slot", C.c_void_p), ("pos", C.c_void_p)]


# every symbol include/gft.h declares: (restype, argtypes)
_vp, _u32, _u64, _i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
SYMBOLS = {
    "gft_engine_create": (_i, [C.POINTER(_vp), _i]),
    "gft_engine_destroy": (None, [_vp]),
    "gft_engine_create_multi": (_i, [C.POINTER(_vp), _vp, _i]),
    "gft_n_devices": (_i, [_vp]),
    "gft_gather_mode": (C.c_char_p, [_vp]),
    "gft_build_info": (C.c_char_p, []),
    "gft_device_engine": (_vp, [_vp, _i]),
    "gft_split_docs": (_i, [_vp, _vp, _u64, _vp]),
    "gft_process_device_multi": (_i, [_vp, _vp, _vp, _vp, _u32, _vp]),
    "gft_last_error": (C.c_char_p, [_vp]),
    "gft_set_stream": (_i, [_vp, _vp]),
    "gft_set_cu_margin": (_i, [_vp, C.c_uint32]),
    "gft_build": (_i, [_vp, _vp, _vp, _u32, _u32]),
    "gft_export_tables": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_import_tables": (_i, [_vp, C.c_char_p, _u64]),
    "gft_n_terms": (_u32, [_vp]),
    "gft_n_states": (_u32, [_vp]),
    "gft_last_nonascii": (_i, [_vp]),
    "gft_scan_kernel": (C.c_char_p, [_vp]),
    "gft_debug_scan5_filter": (_i, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "gft_term": (_i, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "gft_term_id": (C.c_int64, [_vp, _vp, _u32]),
    "gft_scan": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftMatches)]),
    "gft_scan_device": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftMatches)]),
    "gft_set_programs": (_i, [_vp, _vp, _vp, _u32, _u32]),
    "gft_n_exprs": (_u32, [_vp]),
    "gft_n_host_exprs": (_u32, [_vp]),
    "gft_process": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftExtra), _vp]),
    "gft_process_again": (_i, [_vp, _u64, C.POINTER(GftExtra), _vp]),
    "gft_process_device": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftExtra), _vp]),
    "gft_process_device_begin": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftExtra), _vp]),
    "gft_process_device_end": (_i, [_vp]),
    "gft_process_device_complete": (_i, [_vp]),
    "gft_set_expr_labels": (_i, [_vp, _vp, _u32]),
    "gft_compact_device": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_process_sparse": (_i, [_vp, _vp, _vp, _u64, _u32, C.POINTER(GftExtra), C.POINTER(GftSparse)]),
    "gft_debug_compact_host": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_finder_n_tags": (_u32, [_vp]),
    "gft_finder_tag": (_i, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "gft_finder_expression_tag_id": (C.c_int64, [_vp, _u32]),
    "gft_finder_process_texts_sparse": (_i, [_vp, _vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "gft_finder_compact_device": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_finder_create": (_i, [C.POINTER(_vp), _i, _i]),
    "gft_finder_create_multi": (_i, [C.POINTER(_vp), _i, _vp, _i]),
    "gft_finder_destroy": (None, [_vp]),
    "gft_finder_last_error": (C.c_char_p, [_vp]),
    "gft_finder_engine": (_vp, [_vp]),
    "gft_finder_set_substring_engine": (_i, [_vp, _vp, _vp, _vp]),
    "gft_finder_set_regex_engine": (_i, [_vp, _vp, _vp, _vp]),
    "gft_finder_add_expression": (_i, [_vp, C.c_char_p, _u64, C.c_char_p, _u64]),
    "gft_finder_n_expressions": (_u32, [_vp]),
    "gft_finder_n_literals": (_u32, [_vp, _i]),
    "gft_finder_literal": (_i, [_vp, _i, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "gft_finder_expression": (_i, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_vp), C.POINTER(_u32),
                                   C.POINTER(_vp), C.POINTER(_u32)]),
    "gft_finder_force_build": (_i, [_vp]),
    "gft_finder_process_text": (_i, [_vp, C.c_char_p, _u64, _vp, _u32, C.POINTER(_u32)]),
    "gft_finder_process_texts": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "gft_finder_last_regex_docs": (_u64, [_vp]),
    "gft_finder_process_device": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "gft_finder_process_device_begin": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "gft_finder_process_device_end": (_i, [_vp]),
    "gft_finder_debug_add_literal": (_i, [_vp, _i, C.c_char_p, _u32]),
    "gft_finder_debug_set_updated": (_i, [_vp, _i, _i]),
    "gft_finder_debug_get_updated": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "gft_group_create": (_i, [C.POINTER(_vp), _vp]),
    "gft_group_destroy": (None, [_vp]),
    "gft_group_last_error": (C.c_char_p, [_vp]),
    "gft_group_add_rule": (_i, [_vp, C.c_char_p, _u64, C.c_char_p, _u64]),
    "gft_group_state": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_process_jsons": (_i, [_vp, _vp, _vp, _u64, C.c_char_p, _u64, C.c_char_p, _u64, _i, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_last_result": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_evaluate": (_i, [_vp, C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_last_batch": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_group_set_schema": (_i, [_vp, _vp, _vp, _u32, C.c_char_p, _u64, C.c_char_p, _u64]),
    "gft_group_n_rule_exprs": (_u32, [_vp]),
    "gft_group_rule_expr": (_i, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_vp), C.POINTER(_u32)]),
    "gft_group_process_records_device": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "gft_group_process_records": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp]),
    "gft_debug_eval_rules": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u64, _vp]),
    "gft_debug_eval_rules_device": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u64, _vp]),
    "gft_group_tag_records_device": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_tag_records": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_tag_jsons_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_tag_jsons_schema": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_tag_jsons_auto": (_i, [_vp, _vp, _vp, _u64, C.c_char_p, _u64, C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_tag_entries": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_tag_entries_device": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_rules_json_device": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_debug_rules_json": (_i, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_group_tags_json_device": (_i, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_debug_tags_json": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_group_json_leaves_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "gft_group_process_jsons_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "gft_group_process_jsons_schema": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_json_last": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_group_json_paths_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_group_process_jsons_auto": (_i, [_vp, _vp, _vp, _u64, C.c_char_p, _u64, C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_json_auto_last": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_emulate_json_paths": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64), C.POINTER(_u64), _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_json_paths_ref": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_debug_json_leaves_ref": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "gft_debug_emulate_json_leaves": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "gft_debug_json_schema_find": (C.c_int64, [_vp, C.c_int64, C.c_char_p, _u32, C.POINTER(C.c_int64)]),
    "gft_group_dsl_parse": (_i, [C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_group_dsl_tokens": (_i, [C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_dsl_parse": (_i, [C.c_char_p, _u64, _i, _vp, _u64, C.POINTER(_u64)]),
    "gft_regex_required_literals": (_i, [C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_dsl_tokens": (_i, [C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_to_lower": (_i, [C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_to_lower_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_debug_lower_rune": (_u32, [_u32]),
    "gft_debug_emulate_to_lower": (_i, [_vp, _vp, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_finder_lowered_batches": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_split_lines_device": (_i, [_vp, _vp, _u64, _u32, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_split_lines": (_i, [_vp, _u64, _u32, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_split_shape": (None, [C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_finder_split_lines_device": (_i, [_vp, _vp, _u64, _u32, _vp, _u64, C.POINTER(_u64)]),
    "gft_select_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_select_docs": (_i, [_vp, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_select_shape": (None, [C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_context_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64,
                                     C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_context_docs": (_i, [_vp, _vp, _u64, _vp, _u32, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64,
                                    C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_context_shape": (None, [C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_finder_context_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u32, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64,
                                            C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_finder_select_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u32, _vp, _vp, _u64, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_route_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "gft_debug_route_docs": (_i, [_vp, _vp, _u64, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "gft_debug_route_shape": (None, [C.POINTER(_u32)]),
    "gft_finder_route_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "gft_hit_spans_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_redact_spans_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32]),
    "gft_debug_witness_terms": (_i, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_hit_spans": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_redact_spans": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u32]),
    "gft_debug_spans_shape": (None, [C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_finder_hit_spans_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "gft_finder_hit_spans_source_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_i)]),
    "gft_map_spans_to_source_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp]),
    "gft_debug_map_spans_to_source": (_i, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "gft_excerpt_spans_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp,
                                     C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_excerpt_spans": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp,
                                    C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_excerpt_shape": (None, [C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_finder_excerpts_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _i, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp,
                                       C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)]),
    "gft_excerpt_spans_snap_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp,
                                          _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_excerpt_spans_snap": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp,
                                         C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_excerpt_snap_edges": (_i, [_vp, _u64, _u64, _u64, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_finder_excerpts_snap_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _i, _u32, _u32, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _u64,
                                            _vp, _vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)]),
    "gft_mark_spans_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64),
                                  C.POINTER(_u64)]),
    "gft_debug_mark_spans": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(_u64),
                                 C.POINTER(_u64)]),
    "gft_debug_mark_shape": (None, [C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_finder_mark_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _i, _vp, _u32, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp,
                                   C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)]),
    "gft_replace_spans_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _vp,
                                     _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_replace_spans": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp, _vp,
                                    _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "gft_debug_replace_shape": (None, [C.POINTER(_u32)] * 6),
    "gft_finder_replace_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp,
                                      _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_i)]),
    "gft_term_stats_device": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp]),
    "gft_count_columns_device": (_i, [_vp, _vp, _u64, _u32, _vp, _u32, _vp]),
    "gft_batch_term_stats_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _u32, _u64, _vp, _vp, _vp, C.POINTER(_i)]),
    "gft_debug_term_stats": (_i, [_vp, _vp, _u64, _u32, _u32, _u64, _vp, _vp, _vp]),
    "gft_debug_count_columns": (_i, [_vp, _u64, _u32, _vp, _u32, _vp]),
    "gft_debug_stats_shape": (None, [C.POINTER(_u32)] * 8),
    "gft_finder_term_stats_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u32, _u64, _vp, _vp, _vp, C.POINTER(_i)]),
    "gft_score_docs_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _u32, _vp, C.POINTER(_u64)]),
    "gft_top_docs_device": (_i, [_vp, _vp, _u64, _u32, _u64, _vp, _vp, C.POINTER(_u64)]),
    "gft_gather_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_batch_top_docs_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_i)]),
    "gft_batch_top_docs_words_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, C.POINTER(_u64),
                                            C.POINTER(_i)]),
    "gft_debug_score_docs": (_i, [_vp, _vp, _u64, _u32, _vp, _u32, _vp, C.POINTER(_u64)]),
    "gft_debug_top_docs": (_i, [_vp, _u64, _u32, _u64, _vp, _vp, C.POINTER(_u64)]),
    "gft_debug_gather_docs": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, C.POINTER(_u64)]),
    "gft_debug_rank_shape": (None, [C.POINTER(_u32)] * 10),
    "gft_finder_top_docs_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u32, _u32, _u64, _vp, _vp, _vp, C.POINTER(_u64), C.POINTER(_i)]),
    "gft_filter_word_matches_device": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_filter_word_matches": (_i, [_vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_word_rune": (_u32, [_u32]),
    "gft_debug_words_shape": (None, [C.POINTER(_u32)] * 3),
    "gft_scan_words_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "gft_process_words_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "gft_process_words": (_i, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "gft_hit_spans_words_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_batch_term_stats_words_device": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _u32, _u64, _vp, _vp, _vp, C.POINTER(_i)]),
    "gft_finder_set_whole_words": (_i, [_vp, _i]),
    "gft_finder_whole_words": (_i, [_vp]),
    "gft_debug_lowermap_shape": (None, [C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_group_process_json_lines": (_i, [_vp, _vp, _u64, C.c_char_p, _u64, C.c_char_p, _u64, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_emulate_scan": (_i, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _u64, C.POINTER(_u64)]),
    "gft_debug_tables": (_i, [_vp, _vp, _u32, _vp, _u64, _u64, C.c_char_p, C.POINTER(C.c_char_p), _vp, _u64, C.POINTER(_u64), _vp, _u64]),
    "gft_debug_learned_unit": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_debug_last_unit_route": (_i, [_vp, C.POINTER(C.c_char_p)]),
    "gft_debug_last_fold_bits": (_i, [_vp, C.POINTER(_u32)]),
    "gft_debug_scan_plan": (_i, [_vp, _vp, _u32, _u64, C.c_char_p, C.POINTER(C.c_char_p), _vp]),
    "gft_debug_pool_entries": (_i, [_vp, C.POINTER(_u64)]),
    "gft_debug_last_solve_pf": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "gft_debug_judge_batch": (_i, [_vp, _i, _u32, _u64, _u64, _u64, _u64, C.POINTER(_i), C.POINTER(_u64), _vp, _vp, _u64]),
    "gft_debug_learn": (_i, [C.c_char_p, _u32, _i, _u64, _u64, _u64, C.POINTER(_u32), C.POINTER(C.c_double)]),
    "gft_debug_eval_programs": (_i, [_vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "gft_debug_program_shape": (_i, [_vp, _vp, _u32, _u32, _vp, _u32]),
    "gft_debug_plan_solve": (_i, [_u32, _u32, _u32, _i, _u32, _u64, _u32, _u64, _i, _i, _u32, _vp]),
    "gft_debug_plan_solve_pf": (_i, [_u32, _u32, _u32, _i, _u32, _u32, _u64, _u32, _u64, _i, _i, _u32, _u32, _vp]),
    "gft_debug_host_solve": (_i, [_vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_i)]),
    "gft_profile_enable": (_i, [_vp, _i]),
    "gft_profile_read": (_i, [_vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "gft_profile_reset": (_i, [_vp]),
}

EMIT_FN = C.CFUNCTYPE(None, _vp, _vp, _u32, C.c_int64)
BUILD_FN = C.CFUNCTYPE(_i, _vp, _vp, _vp, _u32, _i, _vp, _u32)
FIND_FN = C.CFUNCTYPE(_i, _vp, _vp, _u64, EMIT_FN, _vp, _vp, _u32)

_LIB = None


def _mapped_hip_runtimes():
    """paths of the libamdhip64 copies mapped into this process"""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64.so" in ln})
    except OSError:
        return []


def _hip_runtime_first():
    """libgft.so links /opt/rocm's libamdhip64, PyTorch ships its own copy of the same soname.  Whichever is mapped first
    serves both -- as long as torch comes FIRST: with libgft.so loaded before torch the process has carried two HIP runtimes
    (the one abort in the records).  So a process that can import torch imports it before the library
    is mapped; one without torch has a single runtime anyway.  GFT_NO_TORCH_PRELOAD=1 skips this (a caller that never
    imports torch and does not want its start-up time)."""
    import sys
    if "torch" in sys.modules or os.environ.get("GFT_NO_TORCH_PRELOAD"):
        return
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def _check_one_hip_runtime():
    libs = _mapped_hip_runtimes()
    if len(libs) > 1:
        import warnings
        warnings.warn("two HIP runtimes are mapped into this process (%s): device pointers of one are not valid in the "
                      "other -- import torch before gofindthem_amd loads libgft.so" % ", ".join(libs), RuntimeWarning)


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libgft.so is not built (run `python -m gofindthem_amd.build`); "
                               "gofindthem_amd has no CPU fallback for the hot path")
        _hip_runtime_first()
        L = C.CDLL(LIB_PATH)
        _check_one_hip_runtime()
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)            # AttributeError if a declared symbol is not exported
            f.restype, f.argtypes = res, args
        _LIB = L
    return _LIB
