"""The C ABI of liblc_regex_gpu.so (include/*.h) as ctypes sees it: the structures and callback types, each once, and PROTOTYPES, the
one table of every lc_* function's return and argument types.  bind(L) applies the table to a loaded library -- the real one, the
refshape build or a host double of the tests -- so every library in a process holds the very same type objects.
tests/test_abi_table.py holds the table to the headers and to the library's exports.

Conventions: handles and buffers are c_void_p, text is c_char_p, a malloc'ed string comes back as c_void_p (the caller reads it with
string_at and releases it), an out-scalar is a POINTER to its type, the alarm sink and the clock travel as c_void_p (callers cast)."""
import ctypes

vp, cp, sz, P = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER
i32, u32, i64, u64, u8 = ctypes.c_int, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint8

# lc_alarm_sink_t(user, kind, message, length) and lc_clock_t(user) -> epoch seconds
ALARM_SINK = ctypes.CFUNCTYPE(None, vp, i32, P(ctypes.c_char), sz)
CLOCK = ctypes.CFUNCTYPE(i64, vp)

APSARA_OUT_KEYS = ("status", "secs", "nanos", "base", "npairs", "pairs")
CLOG_OUT_KEYS = ("status", "flags", "spans", "rewrite_begin")
PROM_OUT_KEYS = ("status", "flags", "name", "value", "value_span", "time_span", "secs", "nanos", "nlabels", "labels")
TS_OUT_KEYS = ("status", "secs", "nanos", "matched", "frac_len", "same_as_prev")


class LcRegexInfo(ctypes.Structure):
    _fields_ = [("engine", i32), ("mark_count", i32), ("positions", u32), ("states", u32), ("classes", u32), ("registers", u32),
                ("table_bytes", u32)]


class LcSpanFilter(ctypes.Structure):
    _fields_ = [("re", vp), ("group", u32)]


class LcMatchJob(ctypes.Structure):
    _fields_ = [("re", vp), ("d_data", vp), ("d_off", vp), ("d_len", vp), ("sep_bytes", u32), ("n", u32), ("ngroups", u32),
                ("d_caps", vp), ("d_status", vp)]


class LcColumnar(ctypes.Structure):
    _fields_ = [("n_events", u32), ("n_keys", u32), ("keys", P(cp)), ("key_len", P(u32)), ("base", P(vp)), ("base_len", P(u32)),
                ("spans", P(ctypes.c_int32)), ("state", P(u8)), ("content_bytes", P(u64))]


class LcDesensStats(ctypes.Structure):
    _fields_ = [("rounds", u32), ("pass_through", u32), ("searches", u64)]


class LcMlRecord(ctypes.Structure):
    _fields_ = [("begin", u32), ("length", u32), ("matched", u32)]


class LcJsonMember(ctypes.Structure):
    _fields_ = [("key_begin", u32), ("key_end", u32), ("val_begin", u32), ("val_end", u32), ("type", u8), ("reserved", u8 * 3)]


# the out-structs of the engine entries: every field is the address of the caller's array (device or host memory)
class LcApsaraOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in APSARA_OUT_KEYS]


class LcClogOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in CLOG_OUT_KEYS]


class LcPromOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in PROM_OUT_KEYS]


class LcTsOut(ctypes.Structure):
    _fields_ = [(k, vp) for k in TS_OUT_KEYS]


# name -> (restype, [argtypes]), in the order of the headers
PROTOTYPES = {
    # ---- include/lc_apsara.h
    "lc_apsara_parse_device": (i32, [vp, vp, u32, u32, P(LcApsaraOut), vp]),
    "lc_apsara_parse_host": (i32, [vp, vp, u32, u32, P(LcApsaraOut)]),
    "lc_apsara_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_apsara_processor_create_with_clock": (i32, [cp, vp, vp, P(vp), cp, sz]),
    "lc_apsara_processor_destroy": (None, [vp]),
    "lc_apsara_processor_warnings": (vp, [vp]),
    "lc_apsara_processor_zone_offset": (i32, [vp]),
    "lc_apsara_processor_process": (i32, [vp, vp]),
    "lc_apsara_processor_process_native": (i32, [vp, vp]),
    "lc_apsara_processor_set_clock": (None, [vp, vp, vp]),
    "lc_apsara_processor_set_discard": (None, [vp, i32, i32]),
    "lc_apsara_processor_set_first_trip_pairs": (None, [vp, u32]),
    "lc_apsara_processor_counters": (i32, [vp, P(u64)]),
    "lc_apsara_processor_history_failures": (u64, [vp]),
    "lc_apsara_processor_replayed_lines": (None, [vp, P(u64)]),
    "lc_apsara_processor_set_alarm_sink": (None, [vp, vp, vp]),
    # ---- include/lc_container_log.h
    "lc_container_log_parse_device": (i32, [i32, vp, vp, u32, P(LcClogOut), vp, vp]),
    "lc_container_log_parse_host": (i32, [i32, vp, vp, u32, P(LcClogOut), vp, P(u64)]),
    "lc_container_log_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_container_log_processor_destroy": (None, [vp]),
    "lc_container_log_processor_warnings": (vp, [vp]),
    "lc_container_log_processor_set_config_name": (None, [vp, cp]),
    "lc_container_log_processor_process": (i32, [vp, vp]),
    "lc_container_log_processor_process_native": (i32, [vp, vp]),
    "lc_container_log_processor_counters": (i32, [vp, P(u64)]),
    "lc_container_log_processor_stream_counts": (None, [vp, P(u64)]),
    "lc_container_log_processor_replayed_lines": (u64, [vp]),
    "lc_container_log_processor_set_alarm_sink": (None, [vp, vp, vp]),
    # ---- include/lc_delimiter.h
    "lc_delim_create": (i32, [cp, u32, u8, i32, u32, P(vp)]),
    "lc_delim_destroy": (None, [vp]),
    "lc_delim_uses_quote": (i32, [vp]),
    "lc_delim_split_device": (i32, [vp, vp, vp, u32, u32, vp, vp, vp, vp]),
    "lc_delim_split_host": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "lc_delimiter_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_delimiter_processor_destroy": (None, [vp]),
    "lc_delimiter_processor_warnings": (vp, [vp]),
    "lc_delimiter_processor_process": (i32, [vp, vp]),
    "lc_delimiter_processor_process_native": (i32, [vp, vp]),
    "lc_delimiter_processor_set_first_trip_columns": (None, [vp, u32]),
    "lc_delimiter_processor_counters": (i32, [vp, P(u64)]),
    "lc_delimiter_processor_set_alarm_sink": (None, [vp, vp, vp]),
    # ---- include/lc_desensitize.h
    "lc_desens_create": (i32, [i32, cp, sz, cp, sz, cp, sz, i32, P(vp), P(i32), cp, sz]),
    "lc_desens_free": (None, [vp]),
    "lc_desens_regex": (vp, [vp]),
    "lc_desens_apply_device": (i32, [vp, vp, vp, vp, u32, vp, vp, vp, u64, P(u64), P(LcDesensStats), vp]),
    "lc_desens_apply_host": (i32, [vp, vp, vp, u32, vp, vp, P(vp), P(LcDesensStats)]),
    "lc_desensitize_create": (i32, [cp, P(vp), cp, sz]),
    "lc_desensitize_destroy": (None, [vp]),
    "lc_desensitize_warnings": (vp, [vp]),
    "lc_desensitize_process": (i32, [vp, vp]),
    "lc_desensitize_process_native": (i32, [vp, vp]),
    "lc_desensitize_counters": (i32, [vp, P(u64)]),
    "lc_desensitize_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_desensitize_engine": (vp, [vp]),
    "lc_desensitize_rounds": (u64, [vp]),
    # ---- include/lc_go_regex.h
    "lc_goregex_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_goregex_free": (None, [vp]),
    "lc_goregex_regex": (vp, [vp]),
    "lc_goregex_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_goregex_free_string": (None, [vp]),
    # ---- include/lc_grok.h
    "lc_grok_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_grok_free": (None, [vp]),
    "lc_grok_wait_ready": (None, [vp]),
    "lc_grok_match_count": (i32, [vp]),
    "lc_grok_expanded": (cp, [vp, i32]),
    "lc_grok_processed": (cp, [vp, cp]),
    "lc_grok_denormalize": (vp, [vp, cp, cp, sz]),
    "lc_grok_literal_index": (i32, [vp, P(vp), P(sz)]),
    "lc_grok_plan_masks_device": (i32, [vp, vp, vp, vp, u32, i32, vp, vp, vp, sz, vp]),
    "lc_grok_screen_blob": (i32, [vp, i32, P(vp), P(sz), P(u32)]),
    "lc_grok_engine": (i32, [vp, i32]),
    "lc_grok_entry_info": (i32, [vp, i32, P(u32)]),
    "lc_grok_key_count": (i32, [vp]),
    "lc_grok_key": (cp, [vp, i32]),
    "lc_grok_column_count": (i32, [vp, i32]),
    "lc_grok_column_key": (i32, [vp, i32, i32]),
    "lc_grok_row_ints": (i32, [vp]),
    "lc_grok_scratch_bytes": (sz, [vp, u32]),
    "lc_grok_match_device": (i32, [vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp, sz, vp]),
    "lc_grok_last_batch_stats": (None, [vp]),
    "lc_grok_combiner_stats": (i32, [vp, vp]),
    "lc_grok_lazy_settle": (i32, [vp, u32]),
    "lc_grok_lazy_stats": (i32, [vp, vp]),
    "lc_grok_match_host": (i32, [vp, vp, vp, vp, u32, vp, P(vp)]),
    "lc_grok_result_arrays": (None, [vp, P(vp), P(vp), P(vp), P(vp)]),
    "lc_grok_result_free": (None, [vp]),
    "lc_grok_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_grok_free_string": (None, [vp]),
    # ---- include/lc_json.h
    "lc_json_walk_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp, vp]),
    "lc_json_walk_host": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp, P(u64)]),
    "lc_json_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_json_processor_destroy": (None, [vp]),
    "lc_json_processor_warnings": (vp, [vp]),
    "lc_json_processor_process": (i32, [vp, vp]),
    "lc_json_processor_process_native": (i32, [vp, vp]),
    "lc_json_processor_set_first_trip_members": (None, [vp, u32]),
    "lc_json_processor_counters": (i32, [vp, P(u64)]),
    "lc_json_processor_set_alarm_sink": (None, [vp, vp, vp]),
    # ---- include/lc_multiline.h
    "lc_multiline_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_multiline_free": (None, [vp]),
    "lc_multiline_is_multiline": (i32, [vp]),
    "lc_multiline_warnings": (cp, [vp]),
    "lc_multiline_patterns": (i32, [vp]),
    "lc_multiline_split_host": (i32, [vp, cp, u32, P(P(LcMlRecord)), P(u32), P(u32)]),
    "lc_multiline_free_records": (None, [P(LcMlRecord)]),
    "lc_multiline_bounds_device": (i32, [u32, vp, vp, vp, vp, u32, vp, u32, vp, vp, u32, vp, vp]),
    "lc_multiline_bounds_model": (i32, [u32, vp, u32, vp, u32, vp, u32, vp]),
    "lc_multiline_process_group": (i32, [vp, vp]),
    "lc_multiline_counters": (i32, [vp, P(u64)]),
    "lc_merge_multiline_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_merge_multiline_free": (None, [vp]),
    "lc_merge_multiline_patterns": (i32, [vp]),
    "lc_merge_multiline_warnings": (cp, [vp]),
    "lc_merge_multiline_process_group": (i32, [vp, vp]),
    "lc_merge_multiline_counters": (i32, [vp, P(u64)]),
    # ---- include/lc_processor.h
    "lc_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_processor_destroy": (None, [vp]),
    "lc_processor_key_count": (i32, [vp]),
    "lc_processor_key": (cp, [vp, i32]),
    "lc_processor_process": (i32, [vp, vp]),
    "lc_processor_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_processor_counters": (i32, [vp, P(u64)]),
    "lc_group_from_json": (vp, [cp, cp, sz]),
    "lc_processor_parse_columnar": (i32, [vp, vp, P(P(LcColumnar))]),
    "lc_columnar_free": (None, [P(LcColumnar)]),
    "lc_group_from_lines": (vp, [vp, vp, vp, u32, cp]),
    "lc_group_from_buffer": (vp, [vp, sz, cp, u64, cp]),
    "lc_group_set_metadata": (i32, [vp, cp, cp]),
    "lc_group_to_json": (vp, [vp]),
    "lc_group_event_count": (sz, [vp]),
    "lc_group_new": (vp, []),
    "lc_group_add_raw_event": (i32, [vp, cp, sz]),
    "lc_group_add_log_event": (i32, [vp, cp, cp]),
    "lc_group_event_type": (i32, [vp, sz]),
    "lc_group_event_timestamp": (i32, [vp, sz, P(i64), P(u32), P(i32)]),
    "lc_group_metric_name": (i32, [vp, sz, P(vp), P(sz)]),
    "lc_group_metric_value_bits": (i32, [vp, sz, P(u64)]),
    "lc_group_metric_tag_count": (sz, [vp, sz]),
    "lc_group_metric_tag": (i32, [vp, sz, sz, P(vp), P(sz), P(vp), P(sz)]),
    "lc_group_content_address": (u64, [vp, sz, cp]),
    "lc_group_native": (vp, [vp]),
    "lc_group_free": (None, [vp]),
    "lc_free": (None, [vp]),
    "lc_pipeline_create": (i32, [cp, P(vp), cp, sz]),
    "lc_pipeline_destroy": (None, [vp]),
    "lc_pipeline_is_fused": (i32, [vp]),
    "lc_pipeline_process": (i32, [vp, vp]),
    "lc_pipeline_counters": (i32, [vp, P(u64), P(u64)]),
    "lc_filter_create": (i32, [cp, P(vp), cp, sz]),
    "lc_filter_destroy": (None, [vp]),
    "lc_filter_mode": (i32, [vp]),
    "lc_filter_process": (i32, [vp, vp]),
    "lc_filter_counters": (None, [vp, P(u64)]),
    "lc_filter_none_utf8": (i32, [cp, sz, i32]),
    # ---- include/lc_prom.h
    "lc_prom_parse_device": (i32, [i32, vp, vp, u32, P(LcPromOut), u32, vp]),
    "lc_prom_parse_host": (i32, [i32, vp, vp, u32, P(LcPromOut), u32, P(u64)]),
    "lc_prom_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_prom_processor_destroy": (None, [vp]),
    "lc_prom_processor_warnings": (vp, [vp]),
    "lc_prom_processor_set_config_name": (None, [vp, cp]),
    "lc_prom_processor_process": (i32, [vp, vp]),
    "lc_prom_processor_process_native": (i32, [vp, vp]),
    "lc_prom_processor_counters": (i32, [vp, P(u64)]),
    "lc_prom_processor_deferred_tokens": (u64, [vp]),
    "lc_prom_processor_mop_up_lines": (u64, [vp]),
    "lc_prom_processor_set_first_trip_labels": (None, [vp, u32]),
    "lc_prom_processor_set_alarm_sink": (None, [vp, vp, vp]),
    # ---- include/lc_regex_gpu.h
    "lc_regex_compile": (i32, [cp, sz, u32, i32, P(vp), cp, sz]),
    "lc_regex_free": (None, [vp]),
    "lc_regex_mark_count": (i32, [vp]),
    "lc_regex_group_name": (cp, [vp, i32]),
    "lc_regex_info": (i32, [vp, P(LcRegexInfo)]),
    "lc_regex_table": (i32, [vp, i32, P(vp), P(sz)]),
    "lc_regex_lazy_train": (i32, [vp, vp, vp, vp, u32, vp]),
    "lc_regex_compile_screen": (vp, [cp, sz, u32, u32, sz]),
    "lc_regex_compile_relaxed_screen": (vp, [cp, sz, u32, u32, sz]),
    "lc_regex_screen_device": (i32, [vp, vp, vp, vp, u32, vp, vp, vp, vp]),
    "lc_regex_required_literal": (vp, [vp, P(sz)]),
    "lc_regex_run_captures": (i32, [vp, vp, vp, i32]),
    "lc_regex_atomic_groups": (None, [vp, P(u32), P(u32)]),
    "lc_runtime_set_table_cache_dir": (i32, [cp]),
    "lc_runtime_table_cache_stats": (None, [vp]),
    "lc_runtime_table_cache_stamp": (cp, []),
    "lc_regex_prefer_wave_tdfa": (i32, [vp]),
    "lc_device_count": (i32, []),
    "lc_runtime_prefer_hw_queues": (i32, [i32]),
    "lc_runtime_set_bind_policy": (i32, [i32, i32]),
    "lc_runtime_bind_policy": (i32, []),
    "lc_runtime_bind_thread": (i32, [i32]),
    "lc_runtime_set_thread_device": (i32, [i32]),
    "lc_runtime_thread_device": (i32, []),
    "lc_runtime_device_for_ordinal": (i32, [u32, i32]),
    "lc_regex_match_device": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp]),
    "lc_regex_match_device_engine": (i32, [vp, i32, vp, vp, vp, u32, u32, u32, vp, vp, vp]),
    "lc_regex_match_device_from": (i32, [vp, i32, vp, vp, vp, u32, u32, vp, vp, vp, u32, vp, vp, vp]),
    "lc_regex_match_device_multi": (i32, [vp, u32, vp]),
    "lc_regex_match_device_dyn": (i32, [vp, i32, vp, vp, u32, vp, u32, u32, vp, vp, vp]),
    "lc_sched_scratch_bytes": (sz, [u32]),
    "lc_regex_match_device_ragged": (i32, [vp, i32, vp, vp, vp, u32, u32, vp, u32, vp, vp, vp, sz, vp]),
    "lc_split_scratch_bytes": (sz, [u64]),
    "lc_split_lines_device": (i32, [vp, u64, u8, vp, u32, vp, vp, sz, vp]),
    "lc_upload_pinned": (i32, [vp, vp, sz, vp]),
    "lc_regex_prepare_span_filter": (i32, [vp]),
    "lc_span_filter_device": (i32, [vp, u32, vp, vp, u32, vp, u32, u32, vp, vp, vp, u32, vp, vp]),
    "lc_regex_match_host": (i32, [vp, vp, vp, vp, u32, u32, vp, vp]),
    "lc_regex_match_host_views": (i32, [vp, vp, vp, u32, u32, vp, vp]),
    "lc_gave_up_values_total": (u64, []),
    "lc_last_error": (cp, []),
    "lc_thread_release": (None, []),
    "lc_decide_stats": (i32, [vp]),
    "lc_dfs_stats": (i32, [P(u64)]),
    "lc_nfa_set_dfs": (None, [i32]),
    "lc_launched_kernels": (sz, [cp, sz]),
    # ---- include/lc_timestamp.h
    "lc_strptime_create": (i32, [cp, P(vp), cp, sz]),
    "lc_strptime_destroy": (None, [vp]),
    "lc_strptime_program": (u32, [vp, P(u32)]),
    "lc_strptime_parse_spans_device": (i32, [vp, vp, vp, vp, u32, P(LcTsOut), vp]),
    "lc_strptime_parse_captures_device": (i32, [vp, vp, vp, vp, u32, u32, vp, u32, u32, P(LcTsOut), vp]),
    "lc_strptime_parse_host": (i32, [vp, vp, vp, u32, P(LcTsOut)]),
    "lc_timestamp_zone_seconds": (i64, [i64, i32]),
    "lc_timestamp_zone_reset": (None, []),
    "lc_timestamp_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_timestamp_processor_destroy": (None, [vp]),
    "lc_timestamp_processor_warnings": (vp, [vp]),
    "lc_timestamp_processor_zone_offset": (i32, [vp]),
    "lc_timestamp_processor_process": (i32, [vp, vp]),
    "lc_timestamp_processor_process_native": (i32, [vp, vp]),
    "lc_timestamp_processor_create_with_clock": (i32, [cp, vp, vp, P(vp), cp, sz]),
    "lc_timestamp_processor_set_clock": (None, [vp, vp, vp]),
    "lc_timestamp_processor_set_discard": (None, [vp, i32, i32, i32]),
    "lc_timestamp_processor_set_plain_walk": (None, [vp, i32]),
    "lc_timestamp_processor_walk_stats": (None, [vp, P(u64)]),
    "lc_timestamp_processor_counters": (i32, [vp, P(u64)]),
    "lc_timestamp_processor_history_failures": (u64, [vp]),
    "lc_timestamp_processor_set_alarm_sink": (None, [vp, vp, vp]),
}

# liblc_kvsplit.so (include/kvsplit/lc_kvsplit.h): a table of its own, for a library that stands beside liblc_regex_gpu.so;
# tests/test_kv_abi.py holds it to its header and to that library's exports
KVSPLIT_PROTOTYPES = {
    "lc_kvsplit_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_kvsplit_free": (None, [vp]),
    "lc_kvsplit_device": (i32, [vp, vp, vp, u32, u32, vp, vp, vp, vp]),
    "lc_kvsplit_host": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "lc_kvsplit_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_kvsplit_free_string": (None, [vp]),
    "lc_kvsplit_counters": (i32, [vp, P(u64)]),
    "lc_kvsplit_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_kvsplit_set_first_trip_pairs": (None, [vp, u32]),
    "lc_kvsplit_thread_release": (None, []),
}

# liblc_csv.so (include/csv/lc_csv.h): the same again for the CSV decoder; tests/test_csv_abi.py holds it to its header and exports
CSV_PROTOTYPES = {
    "lc_csv_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_csv_free": (None, [vp]),
    "lc_csv_device": (i32, [vp, vp, vp, u32, u32, vp, vp, vp, vp]),
    "lc_csv_host": (i32, [vp, vp, vp, u32, u32, vp, vp, vp]),
    "lc_csv_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_csv_free_string": (None, [vp]),
    "lc_csv_counters": (i32, [vp, P(u64)]),
    "lc_csv_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_csv_set_first_trip_fields": (None, [vp, u32]),
    "lc_csv_thread_release": (None, []),
}

# liblc_sls.so (include/sls/lc_sls.h): the same again for the SLS encoder; tests/test_sls_abi.py holds it to its header and exports
SLS_PROTOTYPES = {
    "lc_sls_plan_create": (i32, [P(cp), P(u32), u32, P(u32), u32, P(u32), u32, P(vp), cp, sz]),
    "lc_sls_plan_free": (None, [vp]),
    "lc_sls_scratch_bytes": (sz, [u32]),
    "lc_sls_encode_device": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, i32, vp, u64, vp, vp, sz, vp]),
    "lc_sls_match_encode_host": (i32, [vp, vp, vp, vp, u32, vp, vp, i32, P(vp), P(sz), vp, vp]),
    "lc_sls_append_tags": (i32, [P(cp), P(u32), P(cp), P(u32), u32, vp, sz, P(sz)]),
    "lc_sls_thread_release": (None, []),
    "lc_sls_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_sls_processor_destroy": (None, [vp]),
    "lc_sls_processor_serialize": (i32, [vp, vp, i32, P(vp), P(sz), P(i32)]),
    "lc_sls_serialize_group_host": (i32, [vp, i32, P(vp), P(sz)]),
    "lc_sls_processor_counters": (i32, [vp, P(u64), P(u64)]),
}

# liblc_anchor.so (include/anchor/lc_anchor.h): the same again for the anchor processor; tests/test_anchor_abi.py holds it to its header
# and exports
ANCHOR_PROTOTYPES = {
    "lc_anchor_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_anchor_free": (None, [vp]),
    "lc_anchor_stride": (u32, [vp]),
    "lc_anchor_locate_device": (i32, [vp, vp, vp, u32, vp, vp]),
    "lc_anchor_locate_host": (i32, [vp, vp, vp, u32, vp]),
    "lc_anchor_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_anchor_free_string": (None, [vp]),
    "lc_anchor_counters": (i32, [vp, P(u64)]),
    "lc_anchor_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_anchor_thread_release": (None, []),
}

# liblc_lz4.so (include/lz4/lc_lz4.h): the same again for the LZ4 block writer; tests/test_lz4_abi.py holds it to its header and exports
LZ4_PROTOTYPES = {
    "lc_lz4_create": (i32, [u32, P(vp), cp, sz]),
    "lc_lz4_free": (None, [vp]),
    "lc_lz4_chunk_bytes": (u32, [vp]),
    "lc_lz4_bound": (u64, [u64]),
    "lc_lz4_scratch_bytes": (sz, [vp, u64, u32]),
    "lc_lz4_compress_device": (i32, [vp, vp, vp, vp, u32, vp, u64, vp, vp, sz, vp]),
    "lc_lz4_compress_host": (i32, [vp, vp, vp, u32, P(vp), vp]),
    "lc_lz4_match_encode_compress_host": (i32, [vp, vp, vp, vp, vp, u32, vp, vp, i32, vp, u32, P(vp), P(sz), P(u64), vp, vp]),
    "lc_lz4_thread_release": (None, []),
}

# liblc_jsonl.so (include/jsonl/lc_jsonl.h): the same again for the JSON-lines encoder; tests/test_jsonl_abi.py holds it to its header and
# exports
JSONL_PROTOTYPES = {
    "lc_jsonl_plan_create": (i32, [P(cp), P(u32), u32, P(u32), u32, P(u32), u32, P(vp), cp, sz]),
    "lc_jsonl_plan_free": (None, [vp]),
    "lc_jsonl_head": (i32, [P(cp), P(u32), P(cp), P(u32), u32, vp, sz, P(sz)]),
    "lc_jsonl_scratch_bytes": (sz, [vp, u32]),
    "lc_jsonl_encode_device": (i32, [vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, u32, vp, u64, vp, vp, sz, vp]),
    "lc_jsonl_match_encode_host": (i32, [vp, vp, vp, vp, u32, vp, vp, u32, P(vp), P(sz), vp, vp]),
    "lc_jsonl_thread_release": (None, []),
    "lc_jsonl_processor_create": (i32, [cp, P(vp), cp, sz]),
    "lc_jsonl_processor_destroy": (None, [vp]),
    "lc_jsonl_processor_serialize": (i32, [vp, vp, P(vp), P(sz), P(i32)]),
    "lc_jsonl_serialize_group_host": (i32, [vp, P(vp), P(sz)]),
    "lc_jsonl_processor_counters": (i32, [vp, P(u64), P(u64)]),
}

# liblc_strrep.so (include/strrep/lc_strrep.h): the same again for the string-replace processor; tests/test_strrep_abi.py holds it to its
# header and exports
STRREP_PROTOTYPES = {
    "lc_strrep_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_strrep_free": (None, [vp]),
    "lc_strrep_apply_device": (i32, [vp, vp, vp, u32, vp, vp, vp, u64, P(u64), vp]),
    "lc_strrep_apply_host": (i32, [vp, vp, vp, u32, vp, vp, P(vp)]),
    "lc_strrep_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_strrep_free_string": (None, [vp]),
    "lc_strrep_counters": (i32, [vp, P(u64)]),
    "lc_strrep_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_strrep_thread_release": (None, []),
}

# liblc_codec.so (include/codec/lc_codec.h): the same again for the field codecs (base64 encode / decode, MD5); tests/test_codec_abi.py
# holds it to its header and exports
CODEC_PROTOTYPES = {
    "lc_codec_create": (i32, [cp, sz, P(vp), cp, sz]),
    "lc_codec_free": (None, [vp]),
    "lc_codec_apply_device": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, vp, u64, P(u64), vp]),
    "lc_codec_apply_host": (i32, [vp, vp, vp, u32, vp, vp, vp, vp, P(vp)]),
    "lc_codec_set_trip_bytes": (u64, [sz]),
    "lc_codec_process_logs_json": (i32, [vp, cp, sz, P(vp)]),
    "lc_codec_free_string": (None, [vp]),
    "lc_codec_counters": (i32, [vp, P(u64)]),
    "lc_codec_set_alarm_sink": (None, [vp, vp, vp]),
    "lc_codec_thread_release": (None, []),
}


def bind(L, extra=None):
    """restype / argtypes of every table entry (and of `extra`, a table of the same form) that L exports; -> L"""
    for table in (PROTOTYPES, extra or {}):
        for name, (restype, argtypes) in table.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if table is PROTOTYPES:
                    continue
                raise
            fn.restype, fn.argtypes = restype, argtypes
    return L
