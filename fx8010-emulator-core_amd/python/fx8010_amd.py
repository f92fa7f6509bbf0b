"""ctypes binding of libfx8010_amd.so (the C ABI in include/fx8010_amd.h).

Used by tests/, bench.py and __graft_entry__.py.  It only marshals arguments: every computation
happens in the HIP kernel behind the C ABI.  There is no fallback — if the library is missing
``load()`` raises, and if no GPU is usable ``Batch(...)`` raises with the library's own message.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (FX8010_AMD_LIB: another build of the same library - the sanitizer build of `make -C csrc asan`, tests/test_host_sanitizers.py)
LIB_PATH = os.environ.get("FX8010_AMD_LIB") or os.path.join(_HERE, "..", "libfx8010_amd.so")

_f32p = C.POINTER(C.c_float)
_lib = None

OPT_TRAM_DANE, OPT_TRAM_ADDR_SHIFT, OPT_TRAM_INTERP = 1, 2, 4  # FX_OPT_* of include/fx8010_amd.h

# selectors of fxb_info / fxp_lower_info
INFO = {
    "num_instructions": 0, "num_registers": 1, "num_lane_regs": 2, "num_uniform_regs": 3, "lds_bytes_per_wg": 4,
    "waves_per_wg": 5, "num_microops": 6, "itram_slots": 7, "xtram_slots": 8, "tram_ops": 9, "multipass": 10,
    "num_shadowed": 11, "num_ccr_live": 12, "device": 13, "grid": 14, "inst_per_lane": 15, "kernel": 16, "num_rows": 17,
    "xlate_code_bytes": 18, "xlate_inlined": 19, "xlate_called": 20, "xlate_unsaturated": 21, "xlate_valu": 22, "xlate_valu_slow": 23, "xlate_valu_clocks": 24, "xlate_vgpr_constants": 25, "xlate_builds": 26, "code_cache_hits": 27, "code_cached": 28, "xlate_background_builds": 29, "xlate_code_hash": 30, "stage_trials": 31, "control_rows": 32,
    "host_staged_blocks": 33, "host_inplace_blocks": 34, "bus_blocks": 35, "meter_launches": 36, "imajor_blocks": 37,
    "instance_words": 38, "instance_gathers": 39, "instance_scatters": 40, "bus_gain_blocks": 41, "bus_tap_blocks": 42, "bus_send_blocks": 43,
    "bus_feed_blocks": 44, "instance_rings": 45, "instance_rotations": 46, "xlate_quiet": 47, "xlate_quiet_left": 48, "gain_list_sets": 49,
    "register_list_sets": 50, "register_list_gets": 51, "xlate_sum_groups": 52, "xlate_sum_links": 53, "xlate_quiet_repairs": 54,
    "tram_list_sets": 55, "tram_list_gets": 56,
    "meter_selects": 57, "meter_list_reads": 58, "meter_list_resets": 59, "track_list_expands": 60,
    "meter_target_launches": 61, "meter_match_selects": 62, "meter_match_bests": 63,
    "meter_level_launches": 64, "meter_level_selects": 65, "meter_level_list_reads": 66,
    "bank_slots": 67, "bank_stores": 68, "bank_recalls": 69, "bank_bytes": 70,
    "meter_ranks": 71, "meter_match_ranks": 72, "meter_level_ranks": 73,
    "meter_tone_launches": 74, "meter_tone_selects": 75, "meter_tone_list_reads": 76, "meter_tone_ranks": 77,
}

BUS_SHARED_IN, BUS_MIX_OUT = 1, 2  # FXB_BUS_* of include/fx8010_amd.h
TRAM_LOGICAL, TRAM_BROADCAST = 1, 2  # FXB_TRAM_* of include/fx8010_amd.h
METER_ENERGY, METER_PEAK, METER_FULL_SCALE, METER_NONFINITE = 0, 1, 2, 3  # FXB_METER_* of include/fx8010_amd.h: the `stat` of meter_select
METER_BELOW = 1
METER_LARGEST = 2  # FXB_METER_LARGEST: the flag of the meter_rank calls (the same bit as MATCH_LARGEST)
METER_TARGET_LOOP = 1  # FXB_METER_TARGET_LOOP: the flag of meter_set_target
MATCH_ERROR, MATCH_CROSS = 0, 1  # FXB_MATCH_*: the `stat` of meter_select_match and meter_best
MATCH_LARGEST = 2  # FXB_MATCH_LARGEST: the flag of meter_best
METER_MAX_TONES = 8  # FXB_METER_MAX_TONES: the tones of meter_set_tones
LEVEL_ENVELOPE, LEVEL_QUIET = 0, 1  # FXB_LEVEL_*: the `stat` of meter_select_level
BANK_BAD_POSITION, BANK_PHASE, BANK_NO_RING = 1, 2, 3  # FXB_BANK_*: the `reason` of bank_status

# every symbol include/fx8010_amd.h declares (tests check that the library exports them all)
SYMBOLS = [
    "fx_create", "fx_destroy", "fx_load_file", "fx_process", "fx_process_block", "fx_set_register", "fx_get_register",
    "fx_instruction_counter", "fx_error_count", "fx_error_desc", "fx_error_row", "fx_control_count", "fx_control_at",
    "fx_meta_get", "fx_set_option", "fxb_set_option", "fxp_set_option", "fx_set_channels", "fx_get_channels", "fx_ready", "fx_last_error", "fx_last_create_error",
    "fxb_create", "fxb_create_sharded", "fxb_create_on_devices", "fxb_shard_count", "fxb_shard_info", "fxb_shard_kernel_ms", "fxb_shard_plan", "fxb_process_block_dev_shards", "fxb_destroy", "fxb_load_file", "fxb_load_text", "fxb_set_register", "fxb_set_register_i",
    "fxb_get_register_i", "fxb_set_registers_list", "fxb_get_registers_list", "fxb_set_register_tracks_list", "fxb_clear_register_tracks_list", "fxb_set_register_track", "fxb_set_register_array", "fxb_get_register_array", "fxb_seed_noise_i", "fxb_prepare", "fxb_state_size", "fxb_save_state", "fxb_load_state", "fxb_get_tram_i", "fxb_get_cursors_i", "fxb_set_tram_list", "fxb_get_tram_list", "fxb_process_block", "fxb_process_block_dev", "fxb_sync",
    "fxb_process_block_pitched", "fxb_process_block_dev_pitched",
    "fxb_bus_groups", "fxb_process_block_bus", "fxb_process_block_bus_dev", "fxb_bus_set_gains", "fxb_bus_get_gains",
    "fxb_bus_set_gains_list", "fxb_bus_set_send_gains_list", "fxb_bus_set_feed_gains_list",
    "fxb_bus_set_taps", "fxb_bus_get_taps", "fxb_process_block_bus_tap", "fxb_process_block_bus_tap_dev",
    "fxb_bus_set_sends", "fxb_bus_set_send_gains", "fxb_bus_get_sends", "fxb_process_block_bus_aux", "fxb_process_block_bus_aux_dev",
    "fxb_bus_set_feeds", "fxb_bus_set_feed_gains", "fxb_bus_get_feeds", "fxb_process_block_bus_feed", "fxb_process_block_bus_feed_dev",
    "fxb_process_block_imajor", "fxb_process_block_imajor_dev",
    "fxb_instance_image_size", "fxb_copy_instances", "fxb_reset_instances", "fxb_save_instances", "fxb_load_instances", "fxb_load_instances_rotated",
    "fxb_bank_create", "fxb_bank_slots", "fxb_bank_store", "fxb_bank_recall", "fxb_bank_put", "fxb_bank_get", "fxb_bank_status",
    "fxb_meter_enable", "fxb_meter_read", "fxb_meter_samples", "fxb_meter_select", "fxb_meter_read_list", "fxb_meter_reset_list",
    "fxb_meter_set_target", "fxb_meter_clear_target", "fxb_meter_target_seek", "fxb_meter_target_pos", "fxb_meter_read_match", "fxb_meter_select_match", "fxb_meter_best",
    "fxb_meter_set_level", "fxb_meter_clear_level", "fxb_meter_get_level", "fxb_meter_read_level", "fxb_meter_read_level_list", "fxb_meter_select_level",
    "fxb_meter_rank", "fxb_meter_rank_match", "fxb_meter_rank_level",
    "fxb_meter_set_tones", "fxb_meter_get_tones", "fxb_meter_clear_tones", "fxb_meter_read_tones", "fxb_meter_read_tones_list", "fxb_meter_select_tone", "fxb_meter_rank_tone",
    "fxb_instruction_counter", "fxb_instruction_counter_i", "fxb_ood_flags", "fxb_error_count", "fxb_error_desc",
    "fxb_error_row", "fxb_control_count", "fxb_control_at", "fxb_meta_get", "fxb_ready", "fxb_last_error", "fxb_tier_note",
    "fxb_last_kernel_ms", "fxb_info", "fxb_device_count", "fxb_version", "fxb_host_alloc", "fxb_host_free",
    "fxp_create", "fxp_destroy", "fxp_load_file", "fxp_load_text", "fxp_num_registers", "fxp_register_name",
    "fxp_register_type", "fxp_register_ioindex", "fxp_register_value", "fxp_num_instructions", "fxp_instruction",
    "fxp_itram_size", "fxp_xtram_size", "fxp_error_count", "fxp_error_desc", "fxp_error_row", "fxp_control_count",
    "fxp_control_at", "fxp_meta_get", "fxp_ready", "fxp_lut", "fxp_lower", "fxp_lower_info", "fxp_translate", "fxp_quiet_plan", "fxp_track_register", "fxp_translate_staged", "fxp_code_hash", "fxp_last_error",
]


def load():
    """dlopen the in-tree library and declare the prototypes; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.abspath(LIB_PATH)
    if not os.path.exists(path):
        raise RuntimeError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C fx8010-emulator-core_amd/csrc`" % path)
    lib = C.CDLL(path)
    vp, cp, i32, i64, f32 = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_float

    def sig(name, res, *args):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = list(args)

    sig("fx_create", vp, i32); sig("fx_destroy", None, vp); sig("fx_load_file", i32, vp, cp)
    sig("fx_process", i32, vp, _f32p, _f32p); sig("fx_process_block", i32, vp, _f32p, _f32p, i32)
    sig("fx_set_register", i32, vp, cp, f32); sig("fx_get_register", f32, vp, cp)
    sig("fx_instruction_counter", i64, vp)
    for pfx in ("fx_", "fxb_", "fxp_"):
        sig(pfx + "set_option", i32, vp, C.c_uint, i32)
    sig("fx_set_channels", None, vp, i32); sig("fx_get_channels", i32, vp); sig("fx_ready", i32, vp)
    sig("fx_last_error", cp, vp); sig("fx_last_create_error", cp)
    sig("fxb_create", vp, i64, i32, i32); sig("fxb_destroy", None, vp)
    sig("fxb_create_sharded", vp, i64, i32, C.c_uint64); sig("fxb_create_on_devices", vp, i64, i32, C.POINTER(C.c_int), i32)
    sig("fxb_shard_count", i32, vp); sig("fxb_shard_info", i32, vp, i32, C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64))
    sig("fxb_shard_plan", i32, i64, i32, C.POINTER(i64), C.POINTER(i64))
    sig("fxb_shard_kernel_ms", f32, vp, i32)
    sig("fxb_prepare", i32, vp, i32, i32); sig("fxb_state_size", i64, vp); sig("fxb_save_state", i32, vp, vp, i64); sig("fxb_load_state", i32, vp, vp, i64)
    sig("fxb_set_tram_list", i32, vp, i32, vp, i64, i32, i32, vp, C.c_uint); sig("fxb_get_tram_list", i32, vp, i32, vp, i64, i32, i32, vp, C.c_uint)
    sig("fxb_get_tram_i", i32, vp, i32, i64, vp, i32); sig("fxb_get_cursors_i", i32, vp, i64, C.POINTER(C.c_int32))
    sig("fxb_process_block_dev_shards", i32, vp, C.POINTER(vp), C.POINTER(vp), i32)
    sig("fxb_load_file", i32, vp, cp); sig("fxb_load_text", i32, vp, cp)
    sig("fxb_set_register", i32, vp, cp, f32); sig("fxb_set_register_i", i32, vp, cp, i64, f32)
    sig("fxb_set_register_track", i32, vp, cp, vp, i32, i32, i32)
    sig("fxb_set_register_array", i32, vp, cp, vp); sig("fxb_get_register_array", i32, vp, cp, vp)
    sig("fxb_get_register_i", f32, vp, cp, i64); sig("fxb_seed_noise_i", i32, vp, i64, C.c_int32, C.c_int32)
    sig("fxb_process_block", i32, vp, _f32p, _f32p, i32)
    sig("fxb_process_block_dev", i32, vp, vp, vp, i32, vp); sig("fxb_sync", i32, vp)
    sig("fxb_process_block_pitched", i32, vp, vp, vp, i32, i64); sig("fxb_process_block_dev_pitched", i32, vp, vp, vp, i32, i64, vp)
    sig("fxb_bus_groups", i64, vp, i64); sig("fxb_process_block_bus", i32, vp, vp, vp, i32, i64, C.c_uint)
    sig("fxb_process_block_bus_dev", i32, vp, vp, vp, i32, i64, C.c_uint, vp)
    sig("fxb_bus_set_gains", i32, vp, vp, i32); sig("fxb_bus_get_gains", i32, vp, vp)
    for name in ("fxb_bus_set_gains_list", "fxb_bus_set_send_gains_list", "fxb_bus_set_feed_gains_list"):
        sig(name, i32, vp, vp, i64, vp, i32)
    sig("fxb_bus_set_taps", i32, vp, vp, i64); sig("fxb_bus_get_taps", i64, vp, vp, i64)
    sig("fxb_process_block_bus_tap", i32, vp, vp, vp, vp, i32, i64, C.c_uint); sig("fxb_process_block_bus_tap_dev", i32, vp, vp, vp, vp, i32, i64, C.c_uint, vp)
    sig("fxb_bus_set_sends", i32, vp, i64, vp, vp, vp); sig("fxb_bus_set_send_gains", i32, vp, vp, i32); sig("fxb_bus_get_sends", i64, vp, vp, vp, i64, vp, vp, i64)
    sig("fxb_process_block_bus_aux", i32, vp, vp, vp, vp, vp, i32, i64, C.c_uint); sig("fxb_process_block_bus_aux_dev", i32, vp, vp, vp, vp, vp, i32, i64, C.c_uint, vp)
    sig("fxb_bus_set_feeds", i32, vp, i64, vp, vp, vp); sig("fxb_bus_set_feed_gains", i32, vp, vp, i32); sig("fxb_bus_get_feeds", i64, vp, vp, vp, i64, vp, vp, i64)
    sig("fxb_process_block_bus_feed", i32, vp, vp, vp, vp, vp, i32, i64, C.c_uint); sig("fxb_process_block_bus_feed_dev", i32, vp, vp, vp, vp, vp, i32, i64, C.c_uint, vp)
    sig("fxb_process_block_imajor", i32, vp, vp, vp, i32, i64, i64); sig("fxb_process_block_imajor_dev", i32, vp, vp, vp, i32, i64, i64, vp)
    sig("fxb_instance_image_size", i64, vp, i64); sig("fxb_copy_instances", i32, vp, vp, vp, i64); sig("fxb_reset_instances", i32, vp, vp, i64)
    sig("fxb_save_instances", i32, vp, vp, i64, vp, i64); sig("fxb_load_instances", i32, vp, vp, i64, vp, i64)
    sig("fxb_load_instances_rotated", i32, vp, vp, i64, vp, i64)
    sig("fxb_bank_create", i32, vp, i64); sig("fxb_bank_slots", i64, vp); sig("fxb_bank_store", i32, vp, vp, vp, i64); sig("fxb_bank_recall", i32, vp, vp, vp, i64)
    sig("fxb_bank_put", i32, vp, vp, i64, vp, i64); sig("fxb_bank_get", i32, vp, vp, i64, vp, i64); sig("fxb_bank_status", i32, vp, vp, vp, vp, i32)
    sig("fxb_set_registers_list", i32, vp, vp, i32, vp, i64, vp); sig("fxb_get_registers_list", i32, vp, vp, i32, vp, i64, vp)
    sig("fxb_set_register_tracks_list", i32, vp, vp, i32, vp, i64, vp, i32, i32, i32); sig("fxb_clear_register_tracks_list", i32, vp)
    sig("fxb_meter_enable", i32, vp, i32); sig("fxb_meter_read", i32, vp, vp, vp, vp, vp, i32); sig("fxb_meter_samples", i64, vp)
    sig("fxb_meter_select", i64, vp, i32, C.c_double, i64, i64, vp, i64, C.c_uint); sig("fxb_meter_read_list", i32, vp, vp, i64, vp, vp, vp, vp, i32); sig("fxb_meter_reset_list", i32, vp, vp, i64)
    sig("fxb_meter_set_target", i32, vp, vp, i64, i64, C.c_uint); sig("fxb_meter_clear_target", i32, vp); sig("fxb_meter_target_seek", i32, vp, i64); sig("fxb_meter_target_pos", i64, vp)
    sig("fxb_meter_read_match", i32, vp, vp, vp, i32); sig("fxb_meter_select_match", i64, vp, i32, C.c_double, i64, i64, vp, i64, C.c_uint); sig("fxb_meter_best", i32, vp, i32, i64, vp, vp, C.c_uint)
    sig("fxb_meter_set_level", i32, vp, f32, f32, C.c_uint); sig("fxb_meter_clear_level", i32, vp); sig("fxb_meter_get_level", i32, vp, vp, vp)
    sig("fxb_meter_read_level", i32, vp, vp, vp, i32); sig("fxb_meter_read_level_list", i32, vp, vp, i64, vp, vp, i32); sig("fxb_meter_select_level", i64, vp, i32, C.c_double, i64, i64, vp, i64, C.c_uint)
    for name in ("fxb_meter_rank", "fxb_meter_rank_match", "fxb_meter_rank_level", "fxb_meter_rank_tone"):
        sig(name, i64, vp, i32, i64, C.c_double, i64, i64, vp, vp, C.c_uint)
    sig("fxb_meter_set_tones", i32, vp, i32, vp, C.c_uint); sig("fxb_meter_get_tones", i32, vp, vp, vp); sig("fxb_meter_clear_tones", i32, vp)
    sig("fxb_meter_read_tones", i32, vp, vp, vp, vp, i32); sig("fxb_meter_read_tones_list", i32, vp, vp, i64, vp, vp, vp, i32); sig("fxb_meter_select_tone", i64, vp, i32, C.c_double, i64, i64, vp, i64, C.c_uint)
    sig("fxb_instruction_counter", i64, vp); sig("fxb_instruction_counter_i", i64, vp, i64)
    sig("fxb_ood_flags", C.c_uint32, vp); sig("fxb_ready", i32, vp); sig("fxb_last_error", cp, vp); sig("fxb_tier_note", i32, vp, C.c_char_p, i32)
    sig("fxb_last_kernel_ms", f32, vp); sig("fxb_info", i64, vp, i32)
    sig("fxb_device_count", i32); sig("fxb_version", cp)
    sig("fxb_host_alloc", vp, i64); sig("fxb_host_free", None, vp)
    for pfx in ("fx_", "fxb_", "fxp_"):
        sig(pfx + "error_count", i32, vp); sig(pfx + "error_desc", cp, vp, i32); sig(pfx + "error_row", i32, vp, i32)
        sig(pfx + "control_count", i32, vp); sig(pfx + "control_at", cp, vp, i32)
        sig(pfx + "meta_get", i32, vp, cp, cp, i32)
    sig("fxp_create", vp, i32); sig("fxp_destroy", None, vp); sig("fxp_load_file", i32, vp, cp); sig("fxp_load_text", i32, vp, cp)
    sig("fxp_num_registers", i32, vp); sig("fxp_register_name", cp, vp, i32); sig("fxp_register_type", i32, vp, i32)
    sig("fxp_register_ioindex", i32, vp, i32); sig("fxp_register_value", f32, vp, i32)
    sig("fxp_num_instructions", i32, vp); sig("fxp_instruction", None, vp, i32, C.POINTER(C.c_int))
    sig("fxp_itram_size", i32, vp); sig("fxp_xtram_size", i32, vp); sig("fxp_ready", i32, vp)
    sig("fxp_lut", C.POINTER(C.c_double), i32, i32); sig("fxp_lower", i32, vp); sig("fxp_lower_info", i64, vp, i32)
    sig("fxp_last_error", cp, vp)
    sig("fxp_translate", i64, vp, i32, i32, vp, i64, C.c_char_p, i64)
    sig("fxp_quiet_plan", i64, vp, i32, C.POINTER(C.c_int32), i64)
    sig("fxp_track_register", i32, vp, cp)
    sig("fxp_translate_staged", i64, vp, i32, i32, i32, i32, vp, i64, C.c_char_p, i64, C.POINTER(C.c_int), C.POINTER(C.c_int), i32)
    sig("fxp_code_hash", i64, vp, i32, i32, C.c_uint)
    _lib = lib
    return lib


def device_count():
    return int(load().fxb_device_count())


class HostBuffer:
    """float32 numpy array in pinned, device-visible host memory (fxb_host_alloc): blocks on such buffers are processed in place"""

    def __init__(self, shape):
        self._lib = load()
        self.shape = tuple(int(v) for v in shape)
        n = int(np.prod(self.shape))
        self._p = self._lib.fxb_host_alloc(n * 4)
        if not self._p:
            raise RuntimeError(self._lib.fx_last_create_error().decode("latin-1"))
        self.array = np.ctypeslib.as_array(C.cast(self._p, _f32p), shape=(n,)).reshape(self.shape)

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.fxb_host_free(self._p)
            self._p = None

    __del__ = close


class _Reports:
    """error list / control list / metadata accessors shared by the three handle kinds"""
    _pfx = ""

    def _call(self, name, *a):
        return getattr(self._lib, self._pfx + name)(self._h, *a)

    def set_option(self, option, on=True):
        """FX_OPT_* (OPT_TRAM_DANE, OPT_TRAM_ADDR_SHIFT, OPT_TRAM_INTERP): behaviour beyond the reference; before loading"""
        rc = self._call("set_option", option, 1 if on else 0)
        if rc != 0:
            raise RuntimeError("set_option(%d) failed: %d" % (option, rc))

    def errors(self):
        return [(self._call("error_desc", i).decode("latin-1"), self._call("error_row", i)) for i in range(self._call("error_count"))]

    def controls(self):
        return [self._call("control_at", i).decode("latin-1") for i in range(self._call("control_count"))]

    def meta(self):
        out = {}
        buf = C.create_string_buffer(1024)
        for k in ("name", "copyright", "created", "engine", "comment", "guid"):
            if self._call("meta_get", k.encode(), buf, 1024):
                out[k] = buf.value.decode("latin-1")
        return out

    def ready(self):
        return bool(self._call("ready"))


class FrontEnd(_Reports):
    """Host-only loader + lowering (fxp_*): no GPU needed."""
    _pfx = "fxp_"

    def __init__(self, channels=1):
        self._lib = load()
        self._h = self._lib.fxp_create(channels)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fxp_destroy(self._h)
            self._h = None

    __del__ = close

    def load_text(self, text):
        return bool(self._lib.fxp_load_text(self._h, text.encode() if isinstance(text, str) else text))

    def load_file(self, path):
        return bool(self._lib.fxp_load_file(self._h, path.encode()))

    def registers(self):
        n = self._lib.fxp_num_registers(self._h)
        return [(self._lib.fxp_register_name(self._h, i).decode("latin-1"), self._lib.fxp_register_type(self._h, i),
                 self._lib.fxp_register_ioindex(self._h, i),
                 int(np.float32(self._lib.fxp_register_value(self._h, i)).view(np.uint32))) for i in range(n)]

    def instructions(self):
        buf = (C.c_int * 8)()
        out = []
        for i in range(self._lib.fxp_num_instructions(self._h)):
            self._lib.fxp_instruction(self._h, i, buf)
            out.append(tuple(buf))
        return out

    def tram_sizes(self):
        return self._lib.fxp_itram_size(self._h), self._lib.fxp_xtram_size(self._h)

    def lower(self):
        return int(self._lib.fxp_lower(self._h))

    def lower_info(self, what):
        return int(self._lib.fxp_lower_info(self._h, INFO[what]))

    def track_register(self, key):
        """translate() from now on generates the code of a batch in which `key` can have a control track"""
        rc = int(self._lib.fxp_track_register(self._h, key.encode()))
        if rc < 0:
            raise RuntimeError("fxp_track_register: %d %s" % (rc, self.last_error()))
        return rc

    def translate(self, vgprs=0, stream=0):
        """gfx950 machine code of the program as the batch path generates it: (code bytes, assembler listing).
        stream: 0 steady fast, 1 steady exact, 2 last-sample fast, 3 last-sample exact, 4 run-once code, 5 steady quiet
        (empty when the program has no quiet loop: quiet_plan() says why), 6 steady quiet with sum groups - what the device runs
        in place of stream 5 where the plan has groups (empty where it has none)."""
        cap, tcap = 1 << 20, 1 << 23
        code = C.create_string_buffer(cap)
        text = C.create_string_buffer(tcap)
        n = int(self._lib.fxp_translate(self._h, int(vgprs), int(stream), code, cap, text, tcap))
        if n < 0:
            raise RuntimeError("fxp_translate: %d %s" % (n, self.last_error()))
        return code.raw[:n], text.value.decode("ascii")

    def quiet_plan(self, vgprs=0):
        """the plan of the quiet loop (fxp_quiet_plan), read-only: in_force, eligible, why, the counts, checked = [(register-file
        row, register name or None, bound)], dropped = record indices whose saturation the quiet loop omits, records = the
        steady stream's records as an (R, 8) uint32 array (w0 handler slot, w2..w4 A / X / Y, w5 R, w6 / w7 flags or INTERP's 1 - X),
        zero_adds_dropped = sorted record indices whose add of a uniform +0 the quiet loop does not emit,
        sum_groups = [{row, threshold, first, last, watch_start, start_reg, start_bound, links, watched, negate, addend_row,
        addend_reg, dst_reg, addend_bound}] (fx_xlate.hpp SumGroup: per-link lists; links = record indices; the bounds are the
        plan's running bounds of the chain's start and of every addend), sum_links = the links in them"""
        n = int(self._lib.fxp_quiet_plan(self._h, int(vgprs), None, 0))
        if n < 0:
            raise RuntimeError("fxp_quiet_plan: %d %s" % (n, self.last_error()))
        buf = (C.c_int32 * n)()
        self._lib.fxp_quiet_plan(self._h, int(vgprs), buf, n)
        why = self.last_error()
        w = np.frombuffer(buf, dtype=np.int32).copy()
        c, d, r = int(w[6]), int(w[7]), int(w[8])
        names = [self._lib.fxp_register_name(self._h, i).decode("latin-1") for i in range(self._lib.fxp_num_registers(self._h))]
        rows = w[9: 9 + 3 * c].reshape(c, 3)
        checked = [(int(a), names[b] if 0 <= b < len(names) else None, float(np.array([v], dtype=np.int32).view(np.float32)[0])) for a, b, v in rows]
        at = 9 + 3 * c
        z = at + d + 8 * r
        g = z + 1 + int(w[z])
        groups, q = [], g + 2
        for _ in range(int(w[g])):
            row, bits, n, flags, start, sbits = (int(v) for v in w[q: q + 6])
            per = w[q + 6: q + 6 + 7 * n].reshape(n, 7)
            f32 = lambda v: float(np.array([v], dtype=np.int32).view(np.float32)[0])   # noqa: E731
            groups.append({"row": row, "threshold": float(np.array([bits], dtype=np.int32).view(np.float32)[0]), "first": bool(flags & 1), "last": bool(flags & 2),
                           "watch_start": bool(flags & 4), "start_reg": start, "links": [int(v) for v in per[:, 0]], "watched": [bool(v) for v in per[:, 1]],
                           "negate": [bool(v) for v in per[:, 2]], "addend_row": [int(v) for v in per[:, 3]], "addend_reg": [int(v) for v in per[:, 4]],
                           "dst_reg": [int(v) for v in per[:, 5]], "addend_bound": [f32(v) for v in per[:, 6]], "start_bound": f32(sbits)})
            q += 6 + 7 * n
        return {"sum_groups": groups, "sum_links": int(w[g + 1]), "zero_adds_dropped": [int(v) for v in w[z + 1: z + 1 + int(w[z])]], "in_force": bool(w[0]), "eligible": bool(w[1]), "why": why, "sites": int(w[2]), "fast_dropped": int(w[3]), "quiet_dropped": int(w[4]),
                "check_instructions": int(w[5]), "checked": checked, "dropped": [int(v) for v in w[at: at + d]],
                "records": w[at + d: at + d + 8 * r].view(np.uint32).reshape(r, 8)}

    def translate_staged(self, stages, stage=0, stream=0, vgprs=0):
        """the program cut into at most `stages` pipeline stages (fx_xlate.hpp StageInfo): (code, listing, actual stages, info)
        of one stream of one stage; info = [cut record, rows handed over] per cut + [LDS bytes]"""
        cap, tcap = 1 << 20, 1 << 23
        code = C.create_string_buffer(cap)
        text = C.create_string_buffer(tcap)
        actual = C.c_int(0)
        info = (C.c_int * 512)()
        n = int(self._lib.fxp_translate_staged(self._h, int(vgprs), int(stages), int(stage), int(stream), code, cap, text, tcap, C.byref(actual), info, 512))
        if n < 0:
            raise RuntimeError("fxp_translate_staged: %d %s" % (n, self.last_error()))
        k = actual.value
        head = 2 * max(k - 1, 0) + (1 if k > 1 else 0)
        self.stage_store = [int(v) for v in info[head + 1: head + 1 + int(info[head])]] if k > 1 else []   # per row: the stage that stores it
        return code.raw[:n], text.value.decode("ascii"), k, [int(v) for v in info[:head]]

    def code_hash(self, vgprs, stages=1, tram_streaming=False, priority_slices=False):
        """fingerprint of the code object a batch would load (fxb_info xlate_code_hash of a batch in that situation);
        priority_slices: what a batch generates when its launch fills the build's wave slots once, two or more per SIMD"""
        v = int(self._lib.fxp_code_hash(self._h, int(vgprs), int(stages), (1 if tram_streaming else 0) | (2 if priority_slices else 0)))
        if v < 0:
            raise RuntimeError("fxp_code_hash: %d %s" % (v, self.last_error()))
        return v

    def last_error(self):
        return self._lib.fxp_last_error(self._h).decode("latin-1")

    @staticmethod
    def lut(kind, exponent):
        p = load().fxp_lut(kind, exponent)
        return np.ctypeslib.as_array(p, shape=(64,)).copy()


def shard_plan(n_instances, n_shards):
    """[(first_instance, count)] of the partition fxb_create_sharded / fxb_create_on_devices would use; None when a shard
    would be empty.  No device needed."""
    lib = load()
    first, count = (C.c_int64 * max(n_shards, 1))(), (C.c_int64 * max(n_shards, 1))()
    if lib.fxb_shard_plan(int(n_instances), int(n_shards), first, count) != 0:
        return None
    return [(int(first[k]), int(count[k])) for k in range(n_shards)]


class Batch(_Reports):
    """N instances of one program on one GPU (fxb_*)."""
    _pfx = "fxb_"

    def __init__(self, n_instances, channels=1, device=-1, devices=None, device_mask=None):
        """device: one HIP ordinal (-1: current).  devices=[...]: one shard per entry (fxb_create_on_devices; an ordinal may
        repeat).  device_mask: one shard per set bit (fxb_create_sharded)."""
        self._lib = load()
        self.n = int(n_instances)
        self.channels = channels
        if devices is not None:
            arr = (C.c_int * len(devices))(*devices)
            self._h = self._lib.fxb_create_on_devices(self.n, channels, arr, len(devices))
        elif device_mask is not None:
            self._h = self._lib.fxb_create_sharded(self.n, channels, C.c_uint64(device_mask))
        else:
            self._h = self._lib.fxb_create(self.n, channels, device)
        if not self._h:
            raise RuntimeError("fxb_create failed: " + self._lib.fx_last_create_error().decode("latin-1"))

    def shards(self):
        """[(device, first_instance, n_instances)] of the batch's shards"""
        out = []
        for k in range(self._lib.fxb_shard_count(self._h)):
            dev, first, cnt = C.c_int(), C.c_int64(), C.c_int64()
            self._check(self._lib.fxb_shard_info(self._h, k, C.byref(dev), C.byref(first), C.byref(cnt)), "shard_info")
            out.append((dev.value, first.value, cnt.value))
        return out

    def shard_kernel_ms(self):
        """HIP-event time of every shard's most recent launch, ms"""
        return [float(self._lib.fxb_shard_kernel_ms(self._h, k)) for k in range(self._lib.fxb_shard_count(self._h))]

    def process_block_dev_shards(self, d_in, d_out, n_samples):
        """d_in / d_out: one device pointer (int) per shard; asynchronous."""
        k = len(d_in)
        a = (C.c_void_p * k)(*[C.c_void_p(p) for p in d_in])
        b = (C.c_void_p * k)(*[C.c_void_p(p) for p in d_out])
        return self._check(self._lib.fxb_process_block_dev_shards(self._h, a, b, n_samples), "process_block_dev_shards")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fxb_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc < 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self._lib.fxb_last_error(self._h).decode("latin-1")))
        return rc

    def load_text(self, text):
        return bool(self._lib.fxb_load_text(self._h, text.encode() if isinstance(text, str) else text))

    def load_file(self, path):
        return bool(self._lib.fxb_load_file(self._h, path.encode()))

    def set_register(self, key, v):
        return self._check(self._lib.fxb_set_register(self._h, key.encode(), C.c_float(v)), "set_register")

    def set_register_i(self, key, inst, v):
        return self._check(self._lib.fxb_set_register_i(self._h, key.encode(), inst, C.c_float(v)), "set_register_i")

    def set_register_array(self, key, values):
        v = np.ascontiguousarray(values, dtype=np.float32)
        assert v.shape == (self.n,)
        return self._check(self._lib.fxb_set_register_array(self._h, key.encode(), v.ctypes.data_as(C.c_void_p)), "set_register_array")

    def set_register_track(self, key, values, period):
        """values: [steps] (one value for all instances) or [steps, N] (per instance); applied by the next process call at
        samples 0, period, 2*period, ..."""
        v = np.ascontiguousarray(values, dtype=np.float32)
        per = v.ndim == 2
        assert v.ndim == 1 or v.shape[1] == self.n
        return self._check(self._lib.fxb_set_register_track(self._h, key.encode(), v.ctypes.data_as(C.c_void_p), int(v.shape[0]), int(period), 1 if per else 0),
                           "set_register_track")

    def get_register_array(self, key):
        v = np.empty(self.n, dtype=np.float32)
        self._check(self._lib.fxb_get_register_array(self._h, key.encode(), v.ctypes.data_as(C.c_void_p)), "get_register_array")
        return v

    def get_register_i(self, key, inst):
        return float(self._lib.fxb_get_register_i(self._h, key.encode(), inst))

    def get_register_bits_i(self, key, inst):
        return int(np.float32(self.get_register_i(key, inst)).view(np.uint32))

    @staticmethod
    def _key_table(keys):
        names = [keys] if isinstance(keys, (str, bytes)) else list(keys)
        table = (C.c_char_p * max(len(names), 1))(*[k.encode() if isinstance(k, str) else k for k in names])
        return table, len(names)

    def set_registers_list(self, keys, instances, values):
        """Registers `keys` of the listed instances only (include/fx8010_amd.h "Register sets by list"): instances are global
        instance numbers, no two alike, values float32 [len(keys), len(instances)], row k for keys[k], as bit patterns.  Leaves the
        handle as one set_register_i per word would; stream-ordered behind the queued blocks - it does not wait for them, sync()
        covers it.  Returns 0, or 1 when a key is no register."""
        table, n_keys = self._key_table(keys)
        lst = self._instance_list(instances)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.size != n_keys * lst.size:
            raise ValueError("set_registers_list: values must be [len(keys), len(instances)]")
        return self._check(self._lib.fxb_set_registers_list(self._h, table, n_keys, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size),
                                                            C.c_void_p(v.ctypes.data) if v.size else None), "set_registers_list")

    def set_register_tracks_list(self, keys, instances, values, first=0, period=1):
        """Arms one list schedule for the next process call (include/fx8010_amd.h "Register tracks by list"): values is float32
        [steps, len(keys), len(instances)] ([steps, len(instances)] for one key given as a string), as bit patterns; step q falls
        due at sample first + q * period, where register keys[k] of instance instances[i] takes values[q, k, i].  The other
        voices keep what they hold; steps beyond the block are dropped.  Returns 0, or 1 when a key is no register."""
        table, n_keys = self._key_table(keys)
        lst = self._instance_list(instances)
        v = np.ascontiguousarray(values, dtype=np.float32)
        per_step = n_keys * lst.size
        if v.ndim < 1 or v.shape[0] < 1 or v.size != v.shape[0] * per_step:
            raise ValueError("set_register_tracks_list: values must be [steps, len(keys), len(instances)]")
        return self._check(self._lib.fxb_set_register_tracks_list(self._h, table, n_keys, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size),
                                                                  C.c_void_p(v.ctypes.data) if v.size else None, int(v.shape[0]), int(first), int(period)),
                           "set_register_tracks_list")

    def clear_register_tracks_list(self):
        """drops every armed list schedule"""
        return self._check(self._lib.fxb_clear_register_tracks_list(self._h), "clear_register_tracks_list")

    def get_registers_list(self, keys, instances):
        """float32 [len(keys), len(instances)]: what get_register_i returns for every (key, instance), bit for bit, with one
        gather on the device.  Synchronous; repeats are allowed.  Raises KeyError when a key is no register."""
        table, n_keys = self._key_table(keys)
        lst = self._instance_list(instances)
        out = np.zeros((n_keys, lst.size), dtype=np.float32)
        rc = self._check(self._lib.fxb_get_registers_list(self._h, table, n_keys, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size),
                                                          C.c_void_p(out.ctypes.data) if out.size else None), "get_registers_list")
        if rc != 0:
            raise KeyError(self.last_error())
        return out

    def seed_noise_i(self, inst, x1, x2):
        return self._check(self._lib.fxb_seed_noise_i(self._h, inst, x1, x2), "seed_noise_i")

    def prepare(self, n_samples, wait=True):
        """generate the code for blocks of n_samples samples now (and wait for the builder thread's follow-ups)"""
        return self._check(self._lib.fxb_prepare(self._h, int(n_samples), 1 if wait else 0), "prepare")

    def save_state(self):
        """the whole batch's state as one image (numpy uint8): registers, latches, delay memory, positions, LFSR, counters"""
        n = int(self._lib.fxb_state_size(self._h))
        if n < 0:
            raise RuntimeError("state_size failed (%d): %s" % (n, self.last_error()))
        buf = np.empty(n, dtype=np.uint8)
        self._check(self._lib.fxb_save_state(self._h, buf.ctypes.data_as(C.c_void_p), n), "save_state")
        return buf

    def load_state(self, image):
        image = np.ascontiguousarray(image, dtype=np.uint8)
        return self._check(self._lib.fxb_load_state(self._h, image.ctypes.data_as(C.c_void_p), image.size), "load_state")

    # ---- per-instance state (include/fx8010_amd.h "Per-instance state"): lists of global instance numbers
    @property
    def instance_words(self):
        """W: 32-bit words of one instance's record (state rows, then iTRAM slots, then xTRAM slots)"""
        return self.info("instance_words")

    @staticmethod
    def _instance_list(v):
        return np.ascontiguousarray(np.atleast_1d(np.asarray(v)), dtype=np.int64)

    def instance_image_size(self, count):
        n = int(self._lib.fxb_instance_image_size(self._h, int(count)))
        if n < 0:
            raise RuntimeError("instance_image_size failed (%d): %s" % (n, self.last_error()))
        return n

    def copy_instances(self, src, dst):
        """instance dst[k] becomes a bit-for-bit copy of src[k] (a source may repeat); stream-ordered, sync() covers it"""
        src, dst = self._instance_list(src), self._instance_list(dst)
        if src.size != dst.size:
            raise ValueError("copy_instances: src and dst must have the same length")
        return self._check(self._lib.fxb_copy_instances(self._h, C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data), src.size), "copy_instances")

    def reset_instances(self, instances):
        """the listed instances take the state of freshly created ones; the delay-line positions are kept; stream-ordered"""
        v = self._instance_list(instances)
        return self._check(self._lib.fxb_reset_instances(self._h, C.c_void_p(v.ctypes.data), v.size), "reset_instances")

    def save_instances(self, instances):
        """an instance image (numpy uint8): a 64-byte header, then one record of instance_words words per listed instance"""
        v = self._instance_list(instances)
        buf = np.empty(self.instance_image_size(v.size), dtype=np.uint8)
        self._check(self._lib.fxb_save_instances(self._h, C.c_void_p(v.ctypes.data), v.size, C.c_void_p(buf.ctypes.data), buf.size), "save_instances")
        return buf

    def load_instances(self, instances, image):
        """the records of an instance image into the listed instances of this handle (same program and options)"""
        v = self._instance_list(instances)
        image = np.ascontiguousarray(image, dtype=np.uint8)
        return self._check(self._lib.fxb_load_instances(self._h, C.c_void_p(v.ctypes.data), v.size, C.c_void_p(image.ctypes.data), image.size), "load_instances")

    def load_instances_rotated(self, instances, image):
        """load_instances at any delay-line position: the delay memory of every record is rotated on the GPU to the positions its
        destination holds (fxb_load_instances_rotated; info("instance_rings") tells which lines can be rotated)"""
        v = self._instance_list(instances)
        image = np.ascontiguousarray(image, dtype=np.uint8)
        return self._check(self._lib.fxb_load_instances_rotated(self._h, C.c_void_p(v.ctypes.data), v.size, C.c_void_p(image.ctypes.data), image.size), "load_instances_rotated")

    # ---- record bank (include/fx8010_amd.h "Record banks"): instance records kept on the GPU, recalled by list
    def bank_create(self, n_slots):
        """a bank of n_slots zero-filled records in device memory of the handle's GPU; replaces an existing bank, 0 frees it"""
        return self._check(self._lib.fxb_bank_create(self._h, int(n_slots)), "bank_create")

    def bank_slots(self):
        return int(self._lib.fxb_bank_slots(self._h))

    def _bank_lists(self, name, slots, instances):
        s, v = self._instance_list(slots), self._instance_list(instances)
        if s.size != v.size:
            raise ValueError("%s: slots and instances must have the same length" % name)
        return s, v

    def bank_store(self, slots, instances):
        """slot slots[k] takes the record of instance instances[k] (instances may repeat, slots may not); stream-ordered"""
        s, v = self._bank_lists("bank_store", slots, instances)
        return self._check(self._lib.fxb_bank_store(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(v.ctypes.data), s.size), "bank_store")

    def bank_recall(self, slots, instances):
        """instance instances[k] takes the record in slot slots[k] under the rule of load_instances_rotated, the rotations worked
        out on the GPU (slots may repeat, destinations may not); stream-ordered, returns once queued.  What the device refuses
        changes nothing and shows in bank_status()."""
        s, v = self._bank_lists("bank_recall", slots, instances)
        return self._check(self._lib.fxb_bank_recall(self._h, C.c_void_p(s.ctypes.data), C.c_void_p(v.ctypes.data), s.size), "bank_recall")

    def bank_put(self, slots, image):
        """the records of an instance image (save_instances, bank_get) into the listed slots, record k into slots[k]; synchronous"""
        s = self._instance_list(slots)
        image = np.ascontiguousarray(image, dtype=np.uint8)
        return self._check(self._lib.fxb_bank_put(self._h, C.c_void_p(s.ctypes.data), s.size, C.c_void_p(image.ctypes.data), image.size), "bank_put")

    def bank_get(self, slots):
        """an instance image (numpy uint8) of the listed slots, as save_instances gives one of instances; synchronous"""
        s = self._instance_list(slots)
        buf = np.empty(self.instance_image_size(s.size), dtype=np.uint8)
        self._check(self._lib.fxb_bank_get(self._h, C.c_void_p(s.ctypes.data), s.size, C.c_void_p(buf.ctypes.data), buf.size), "bank_get")
        return buf

    def bank_status(self, reset=False):
        """(refused_calls, entry, reason) after the queued bank calls: the recalls the device has refused since the last reset, and
        of the most recent one its lowest bad list entry (-1: none) and the reason (BANK_*; 0: none)"""
        refused, entry, reason = C.c_int64(0), C.c_int64(-1), C.c_int(0)
        self._check(self._lib.fxb_bank_status(self._h, C.byref(refused), C.byref(entry), C.byref(reason), 1 if reset else 0), "bank_status")
        return int(refused.value), int(entry.value), int(reason.value)

    def set_tram_list(self, which, instances, first, values, logical=False):
        """A window of delay line `which` (0 iTRAM, 1 xTRAM) of the listed instances only (include/fx8010_amd.h "Delay-line windows
        by list"): instances are global instance numbers, no two alike; values float32 [len(instances), n_words] - row i is the
        window of instances[i], words first .. first + n_words - 1 - or 1-D [n_words], ONE window written to every listed instance.
        logical: the index is the age in the ring (0 = the newest word), resolved per instance on the device; else it is the slot.
        Bit patterns.  Stream-ordered behind the queued blocks - it does not wait for them, sync() covers it."""
        lst = self._instance_list(instances)
        v = np.ascontiguousarray(values, dtype=np.float32)
        if v.ndim == 1:
            flags, n_words = TRAM_BROADCAST, int(v.size)
        elif v.ndim == 2 and v.shape[0] == lst.size:
            flags, n_words = 0, int(v.shape[1])
        else:
            raise ValueError("set_tram_list: values must be [n_words] or [len(instances), n_words]")
        flags |= TRAM_LOGICAL if logical else 0
        return self._check(self._lib.fxb_set_tram_list(self._h, int(which), C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size), int(first), n_words,
                                                       C.c_void_p(v.ctypes.data) if v.size else None, flags), "set_tram_list")

    def get_tram_list(self, which, instances, first, n_words, logical=False):
        """float32 [len(instances), n_words]: the same windows read back, bit for bit, with one gather on the device.  Synchronous;
        repeats are allowed.  Without `logical` row i equals get_tram_i(which, instances[i], ...)[first : first + n_words]."""
        lst = self._instance_list(instances)
        out = np.zeros((lst.size, int(n_words)), dtype=np.float32)
        self._check(self._lib.fxb_get_tram_list(self._h, int(which), C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size), int(first), int(n_words),
                                                C.c_void_p(out.ctypes.data) if out.size else None, TRAM_LOGICAL if logical else 0), "get_tram_list")
        return out

    def get_tram_i(self, which, inst, n_slots):
        out = np.empty(n_slots, dtype=np.float32)
        self._check(self._lib.fxb_get_tram_i(self._h, int(which), int(inst), out.ctypes.data_as(C.c_void_p), int(n_slots)), "get_tram_i")
        return out

    def get_cursors_i(self, inst):
        buf = (C.c_int32 * 4)()
        self._check(self._lib.fxb_get_cursors_i(self._h, int(inst), buf), "get_cursors_i")
        return list(buf)

    def _row_pitch(self, shape, strides):
        """P when strides (in floats) of an [S, channels, N] array walk a [S][channels][P] buffer, else None"""
        S, ch, n = shape
        if (ch, n) != (self.channels, self.n) or strides[2] != 1:
            return None
        if ch > 1:
            p = strides[1]
            return p if p >= n and (S <= 1 or strides[0] == ch * p) else None
        return (strides[0] if strides[0] >= n else None) if S > 1 else n

    def process_block(self, x, out=None):
        """x: float32 [S, N] (mono) or [S, channels, N]; returns the same shape (into `out` when given: e.g. a view of pinned
        memory - large blocks from pinned buffers are copied at DMA rate and overlap with the kernel).  Column slices of a
        larger [S, channels, P] buffer (pin[:, :, lo:hi]) go to the library as they are, x and out with one common P: in place
        when the buffer is pinned."""
        if out is not None and isinstance(x, np.ndarray) and x.ndim == 3 and x.shape[0] > 0:
            def pitch(a):
                ok = isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 3 and all(t % 4 == 0 for t in a.strides)
                return self._row_pitch(a.shape, [t // 4 for t in a.strides]) if ok else None
            px, po = pitch(x), pitch(out)
            if px is not None and px == po and out.flags["WRITEABLE"] and not (x.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"]):
                self._check(self._lib.fxb_process_block_pitched(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), x.shape[0], px),
                            "process_block")
                return out
        x = np.ascontiguousarray(x, dtype=np.float32)
        S = x.shape[0]
        assert x.size == S * self.channels * self.n, "input must be [S, channels, N]"
        if out is None:
            out = np.empty_like(x)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.size == x.size
        self._check(self._lib.fxb_process_block(self._h, x.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p), S), "process_block")
        return out

    def process_block_dev(self, d_in, d_out, n_samples, stream=None):
        """device pointers (ints); asynchronous."""
        return self._check(self._lib.fxb_process_block_dev(self._h, C.c_void_p(d_in), C.c_void_p(d_out), n_samples, C.c_void_p(stream or 0)), "process_block_dev")

    def process_block_dev_pitched(self, d_in, d_out, n_samples, pitch=None, stream=None):
        """d_in / d_out: device pointers (ints) of [n_samples][channels][pitch] floats whose columns 0..N-1 are this handle's
        instances, or torch device tensors [n_samples, channels, N] (column slices of a wider tensor included; the pitch comes
        from stride()).  Buffers the handle's device cannot address are refused without a launch.  Asynchronous."""
        def ptr(t):
            if isinstance(t, int):
                return t, None
            assert t.element_size() == 4 and t.dim() == 3 and tuple(t.shape) == (n_samples, self.channels, self.n), "[S, channels, N] float32"
            p = self._row_pitch(tuple(t.shape), tuple(t.stride()))
            assert p is not None, "rows of one pitch: [S][channels][P]"
            return t.data_ptr(), p
        (a, pa), (b, pb) = ptr(d_in), ptr(d_out)
        p = pitch if pitch is not None else (pa if pa is not None else pb)
        assert p is not None, "pitch: give it with pointers"
        assert pa in (None, p) and pb in (None, p), "d_in and d_out with one common pitch"
        return self._check(self._lib.fxb_process_block_dev_pitched(self._h, C.c_void_p(a), C.c_void_p(b), int(n_samples), int(p), C.c_void_p(stream or 0)),
                           "process_block_dev_pitched")

    def bus_groups(self, group):
        """G = ceil(N / group): the columns of a shared input / a mixed output"""
        return self._check(int(self._lib.fxb_bus_groups(self._h, int(group))), "bus_groups")

    def process_block_bus(self, x, group, shared_in=True, mix_out=True, out=None, tap_out=None, taps=False, aux=False, aux_out=None):
        """A block with a shared input and / or a mixed output per group of `group` consecutive instances.  x: float32
        [S, channels, G] with shared_in (instance n hears column n // group), else [S, channels, N]; returns [S, channels, G] with
        mix_out (every group's sum, in the order include/fx8010_amd.h fixes), else [S, channels, N] (mono: the channel axis may be
        left out).  Into `out` when given; x and out in pinned memory (HostBuffer.array) are read and written in place.
        With taps=True or a tap_out (float32 [S, channels, T], T = len(bus_get_taps()); pinned: stored to in place) the block also
        delivers the tapped instances' own output words, pre-fader, and returns (out, taps).
        With aux=True or an aux_out (float32 [S, channels, A], A the aux buses of bus_set_sends; pinned: stored to in place) the
        block also delivers the sends, pre-fader, and the result gets one more element at its end: (out, aux) or (out, taps, aux)."""
        G = self.bus_groups(group)
        x = np.ascontiguousarray(x, dtype=np.float32)
        S = x.shape[0]
        assert x.size == S * self.channels * (G if shared_in else self.n), "input must be [S, channels, %s]" % ("G" if shared_in else "N")
        shape = ((S,) if x.ndim == 2 else (S, self.channels)) + ((G if mix_out else self.n),)
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.size == int(np.prod(shape))
        flags = (BUS_SHARED_IN if shared_in else 0) | (BUS_MIX_OUT if mix_out else 0)
        if aux_out is not None or aux:
            lead = (S,) if x.ndim == 2 else (S, self.channels)
            A = C.c_int64(0)
            self._check(int(self._lib.fxb_bus_get_sends(self._h, C.byref(A), None, 0, None, None, 0)), "bus_get_sends")
            if aux_out is None:
                aux_out = np.empty(lead + (A.value,), dtype=np.float32)
            assert aux_out.dtype == np.float32 and aux_out.flags["C_CONTIGUOUS"] and aux_out.flags["WRITEABLE"] and aux_out.size == int(np.prod(lead)) * A.value, "aux_out must be [S, channels, A]"
            if tap_out is not None or taps:
                T = int(self._lib.fxb_bus_get_taps(self._h, None, 0))
                if tap_out is None:
                    tap_out = np.empty(lead + (T,), dtype=np.float32)
                assert tap_out.dtype == np.float32 and tap_out.flags["C_CONTIGUOUS"] and tap_out.flags["WRITEABLE"] and tap_out.size == int(np.prod(lead)) * T, "tap_out must be [S, channels, T]"
            self._check(self._lib.fxb_process_block_bus_aux(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(tap_out.ctypes.data) if tap_out is not None else None,
                                                            C.c_void_p(aux_out.ctypes.data), S, int(group), flags), "process_block_bus")
            return (out, aux_out) if tap_out is None else (out, tap_out, aux_out)
        if tap_out is not None or taps:
            T = int(self._lib.fxb_bus_get_taps(self._h, None, 0))
            tshape = ((S,) if x.ndim == 2 else (S, self.channels)) + (T,)
            if tap_out is None:
                tap_out = np.empty(tshape, dtype=np.float32)
            assert tap_out.dtype == np.float32 and tap_out.flags["C_CONTIGUOUS"] and tap_out.flags["WRITEABLE"] and tap_out.size == int(np.prod(tshape)), "tap_out must be [S, channels, T]"
            self._check(self._lib.fxb_process_block_bus_tap(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(tap_out.ctypes.data), S, int(group), flags),
                        "process_block_bus")
            return out, tap_out
        self._check(self._lib.fxb_process_block_bus(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), S, int(group), flags), "process_block_bus")
        return out

    def process_block_bus_dev(self, d_in, d_out, n_samples, group, shared_in=True, mix_out=True, stream=None, d_tap_out=None, d_aux_out=None):
        """d_in / d_out: device pointers (ints) or contiguous float32 torch tensors, [n_samples, channels, G] on a side with its
        flag and [n_samples, channels, N] on the other; single-shard handles; asynchronous on `stream` (a hipStream_t as int).
        d_tap_out: the same for the [n_samples, channels, T] rows of the taps in force (bus_set_taps); d_aux_out: for the
        [n_samples, channels, A] rows of the sends in force (bus_set_sends)."""
        G = self.bus_groups(group)

        def ptr(t, width):
            if isinstance(t, int):
                return t
            assert t.element_size() == 4 and t.is_contiguous() and t.numel() == n_samples * self.channels * width, "[S, channels, %d] float32" % width
            return t.data_ptr()
        a, b = ptr(d_in, G if shared_in else self.n), ptr(d_out, G if mix_out else self.n)
        flags = (BUS_SHARED_IN if shared_in else 0) | (BUS_MIX_OUT if mix_out else 0)
        if d_aux_out is not None:
            A = C.c_int64(0)
            self._check(int(self._lib.fxb_bus_get_sends(self._h, C.byref(A), None, 0, None, None, 0)), "bus_get_sends")
            t = ptr(d_tap_out, int(self._lib.fxb_bus_get_taps(self._h, None, 0))) if d_tap_out is not None else None
            return self._check(self._lib.fxb_process_block_bus_aux_dev(self._h, C.c_void_p(a), C.c_void_p(b), C.c_void_p(t) if t is not None else None, C.c_void_p(ptr(d_aux_out, A.value)),
                                                                        int(n_samples), int(group), flags, C.c_void_p(stream or 0)), "process_block_bus_dev")
        if d_tap_out is not None:
            t = ptr(d_tap_out, int(self._lib.fxb_bus_get_taps(self._h, None, 0)))
            return self._check(self._lib.fxb_process_block_bus_tap_dev(self._h, C.c_void_p(a), C.c_void_p(b), C.c_void_p(t), int(n_samples), int(group), flags,
                                                                        C.c_void_p(stream or 0)), "process_block_bus_dev")
        return self._check(self._lib.fxb_process_block_bus_dev(self._h, C.c_void_p(a), C.c_void_p(b), int(n_samples), int(group), flags, C.c_void_p(stream or 0)),
                           "process_block_bus_dev")

    def bus_set_gains(self, gains, ramp=False):
        """Per-instance gains of the mixed output of bus blocks (include/fx8010_amd.h "Bus gains").  gains: float32 [channels, N] by
        global instance, every value finite ([N] for mono), or None: gains off, the unweighted sum.  ramp: the next block with
        mix_out moves every weight linearly from the gains in force to these, reaching them exactly on its last sample."""
        if gains is None:
            return self._check(self._lib.fxb_bus_set_gains(self._h, None, 0), "bus_set_gains")
        g = np.ascontiguousarray(gains, dtype=np.float32)
        assert g.size == self.channels * self.n, "gains must be [channels, N]"
        return self._check(self._lib.fxb_bus_set_gains(self._h, C.c_void_p(g.ctypes.data), 1 if ramp else 0), "bus_set_gains")

    def _set_gains_list(self, fn, what, indices, gains, ramp):
        lst = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        g = np.ascontiguousarray(gains, dtype=np.float32)
        assert g.size == self.channels * lst.size, "gains must be [channels, len(list)]"
        return self._check(fn(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size), C.c_void_p(g.ctypes.data) if g.size else None, 1 if ramp else 0), what)

    def bus_set_gains_list(self, instances, gains, ramp=False):
        """The gains of the listed instances only (include/fx8010_amd.h "Gain sets by list"): instances are global instance numbers,
        no two alike, gains float32 [channels, len(instances)], column k for instances[k].  ramp: the listed weights move over the
        next block with mix_out (a ramp already pending keeps its start); without it they are in force at once, and a ramp that is
        pending for the other instances stays pending.  Does not wait for queued blocks.  Raises while gains are off."""
        return self._set_gains_list(self._lib.fxb_bus_set_gains_list, "bus_set_gains_list", instances, gains, ramp)

    def bus_get_gains(self):
        """float32 [channels, N]: the gains in force - while a ramp waits for its block the ones it will start from, after that
        block its target.  Synchronous; raises while gains are off."""
        g = np.empty((self.channels, self.n), dtype=np.float32)
        self._check(self._lib.fxb_bus_get_gains(self._h, C.c_void_p(g.ctypes.data)), "bus_get_gains")
        return g

    def bus_set_taps(self, instances):
        """The instances whose own output the next tapped bus blocks deliver beside the mix (include/fx8010_amd.h "Bus taps"): up to
        65 536 global instance numbers in any order, repeats allowed; None or an empty list turns taps off."""
        lst = np.ascontiguousarray([] if instances is None else instances, dtype=np.int64).reshape(-1)
        return self._check(self._lib.fxb_bus_set_taps(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size)), "bus_set_taps")

    def bus_get_taps(self):
        """int64 [T]: the tap list in force (empty while taps are off)"""
        T = self._check(int(self._lib.fxb_bus_get_taps(self._h, None, 0)), "bus_get_taps")
        lst = np.zeros(T, dtype=np.int64)
        if T:
            self._check(int(self._lib.fxb_bus_get_taps(self._h, C.c_void_p(lst.ctypes.data), T)), "bus_get_taps")
        return lst

    def bus_set_sends(self, offsets, members, gains=None):
        """The aux buses the next bus blocks with aux=True deliver beside the mix (include/fx8010_amd.h "Bus sends"): CSR - bus b
        owns members[offsets[b]:offsets[b+1]], global instance numbers in any order, repeats allowed; gains float32 [channels, E]
        (mono: [E]), None for 1.0 everywhere.  offsets None or of one value turns sends off."""
        off = np.ascontiguousarray([0] if offsets is None else offsets, dtype=np.int64).reshape(-1)
        mem = np.ascontiguousarray([] if members is None else members, dtype=np.int64).reshape(-1)
        A = max(int(off.size) - 1, 0)
        g = None
        if gains is not None and A > 0:
            g = np.ascontiguousarray(gains, dtype=np.float32)
            assert g.size == self.channels * int(off[-1]) and mem.size >= int(off[-1]), "gains must be [channels, E]"
        assert A == 0 or mem.size >= int(off[-1]), "members must hold offsets[-1] entries"
        return self._check(self._lib.fxb_bus_set_sends(self._h, A, C.c_void_p(off.ctypes.data), C.c_void_p(mem.ctypes.data) if mem.size else None,
                                                       C.c_void_p(g.ctypes.data) if g is not None else None), "bus_set_sends")

    def bus_set_send_gains(self, gains, ramp=False):
        """New weights [channels, E] for the sends in force; with ramp the next block with aux moves every weight linearly from
        the ones in force to these and ends exactly on them (the state machine of bus_set_gains)."""
        g = np.ascontiguousarray(gains, dtype=np.float32)
        E = self._check(int(self._lib.fxb_bus_get_sends(self._h, None, None, 0, None, None, 0)), "bus_get_sends")
        assert g.size == self.channels * E, "gains must be [channels, E]"
        return self._check(self._lib.fxb_bus_set_send_gains(self._h, C.c_void_p(g.ctypes.data), 1 if ramp else 0), "bus_set_send_gains")

    def bus_set_send_gains_list(self, entries, gains, ramp=False):
        """The weights of the listed entries of the sends in force only: entries index the `members` array (what bus_get_sends
        returns), no two alike, gains float32 [channels, len(entries)].  The rules of bus_set_gains_list; does not wait for queued
        blocks, where bus_set_send_gains does."""
        return self._set_gains_list(self._lib.fxb_bus_set_send_gains_list, "bus_set_send_gains_list", entries, gains, ramp)

    def bus_get_sends(self):
        """(offsets int64 [A + 1], members int64 [E], gains float32 [channels, E]) of the sends in force - the gains are a, as
        bus_get_gains returns them - or (array([0]), empty, empty) while sends are off"""
        A = C.c_int64(0)
        E = self._check(int(self._lib.fxb_bus_get_sends(self._h, C.byref(A), None, 0, None, None, 0)), "bus_get_sends")
        off, mem, g = np.zeros(A.value + 1, dtype=np.int64), np.zeros(E, dtype=np.int64), np.zeros((self.channels, E), dtype=np.float32)
        if A.value:
            self._check(int(self._lib.fxb_bus_get_sends(self._h, None, C.c_void_p(off.ctypes.data), off.size, C.c_void_p(mem.ctypes.data), C.c_void_p(g.ctypes.data), E)), "bus_get_sends")
        return off, mem, g

    def bus_set_feeds(self, n_src, offsets, sources, gains=None):
        """The lists the next feed blocks build every instance's input from (include/fx8010_amd.h "Bus feeds"): CSR by instance -
        instance n owns sources[offsets[n]:offsets[n+1]], columns of a source block [S, channels, n_src], in any order, repeats
        allowed, none allowed; gains float32 [channels, E] (mono: [E]), None for unweighted.  n_src 0 turns feeds off."""
        n_src = int(n_src)
        if n_src == 0:
            return self._check(self._lib.fxb_bus_set_feeds(self._h, 0, None, None, None), "bus_set_feeds")
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        src = np.ascontiguousarray([] if sources is None else sources, dtype=np.int64).reshape(-1)
        assert off.size == self.n + 1 and src.size >= int(off[-1]), "offsets must hold N + 1 values, sources offsets[-1] entries"
        g = None
        if gains is not None:
            g = np.ascontiguousarray(gains, dtype=np.float32)
            assert g.size == self.channels * int(off[-1]), "gains must be [channels, E]"
        return self._check(self._lib.fxb_bus_set_feeds(self._h, n_src, C.c_void_p(off.ctypes.data), C.c_void_p(src.ctypes.data) if src.size else None,
                                                       C.c_void_p(g.ctypes.data) if g is not None and g.size else None), "bus_set_feeds")

    def bus_set_feed_gains(self, gains, ramp=False):
        """New weights [channels, E] for the feeds in force, or None: back to unweighted.  With ramp the next feed block moves every
        weight linearly from the ones in force to these and ends exactly on them (the state machine of bus_set_gains)."""
        if gains is None:
            return self._check(self._lib.fxb_bus_set_feed_gains(self._h, None, 0), "bus_set_feed_gains")
        g = np.ascontiguousarray(gains, dtype=np.float32)
        E = self._check(int(self._lib.fxb_bus_get_feeds(self._h, None, None, 0, None, None, 0)), "bus_get_feeds")
        assert g.size == self.channels * E, "gains must be [channels, E]"
        return self._check(self._lib.fxb_bus_set_feed_gains(self._h, C.c_void_p(g.ctypes.data), 1 if ramp else 0), "bus_set_feed_gains")

    def bus_set_feed_gains_list(self, entries, gains, ramp=False):
        """The weights of the listed entries of the feeds in force only: entries index the `sources` array (what bus_get_feeds
        returns), no two alike, gains float32 [channels, len(entries)].  Unweighted feeds become weighted first, 1.0 everywhere.
        The rules of bus_set_gains_list; does not wait for queued blocks, where bus_set_feed_gains does."""
        return self._set_gains_list(self._lib.fxb_bus_set_feed_gains_list, "bus_set_feed_gains_list", entries, gains, ramp)

    def bus_get_feeds(self):
        """(n_src, offsets int64 [N + 1], sources int64 [E], gains float32 [channels, E]) of the feeds in force - the gains are a,
        1.0 everywhere while the feeds are unweighted - or (0, array([0]), empty, empty) while feeds are off"""
        M = C.c_int64(0)
        E = self._check(int(self._lib.fxb_bus_get_feeds(self._h, C.byref(M), None, 0, None, None, 0)), "bus_get_feeds")
        if M.value == 0:
            return 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros((self.channels, 0), dtype=np.float32)
        off, src, g = np.zeros(self.n + 1, dtype=np.int64), np.zeros(E, dtype=np.int64), np.zeros((self.channels, E), dtype=np.float32)
        self._check(int(self._lib.fxb_bus_get_feeds(self._h, None, C.c_void_p(off.ctypes.data), off.size, C.c_void_p(src.ctypes.data), C.c_void_p(g.ctypes.data), E)), "bus_get_feeds")
        return M.value, off, src, g

    def process_block_bus_feed(self, src, group=1, mix_out=False, out=None, tap_out=None, taps=False, aux=False, aux_out=None):
        """A bus block whose per-instance input is built on the device from the feeds in force (bus_set_feeds).  src: float32
        [S, channels, M] (mono: [S, M]), pinned, pageable or - through process_block_bus_feed_dev - device memory.  Everything else
        as process_block_bus without shared_in: returns out, or (out, taps), (out, aux), (out, taps, aux)."""
        M = C.c_int64(0)
        self._check(int(self._lib.fxb_bus_get_feeds(self._h, C.byref(M), None, 0, None, None, 0)), "bus_get_feeds")
        src = np.ascontiguousarray(src, dtype=np.float32)
        S = src.shape[0]
        assert M.value == 0 or src.size == S * self.channels * M.value, "src must be [S, channels, M]"
        lead = (S,) if src.ndim == 2 else (S, self.channels)
        shape = lead + ((self.bus_groups(group) if mix_out else self.n),)
        if out is None:
            out = np.empty(shape, dtype=np.float32)
        assert out.dtype == np.float32 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.size == int(np.prod(shape))
        if tap_out is None and taps:
            tap_out = np.empty(lead + (int(self._lib.fxb_bus_get_taps(self._h, None, 0)),), dtype=np.float32)
        if aux_out is None and aux:
            A = C.c_int64(0)
            self._check(int(self._lib.fxb_bus_get_sends(self._h, C.byref(A), None, 0, None, None, 0)), "bus_get_sends")
            aux_out = np.empty(lead + (A.value,), dtype=np.float32)
        for side in (tap_out, aux_out):
            assert side is None or (side.dtype == np.float32 and side.flags["C_CONTIGUOUS"] and side.flags["WRITEABLE"])
        self._check(self._lib.fxb_process_block_bus_feed(self._h, C.c_void_p(src.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(tap_out.ctypes.data) if tap_out is not None else None,
                                                         C.c_void_p(aux_out.ctypes.data) if aux_out is not None else None, S, int(group), BUS_MIX_OUT if mix_out else 0), "process_block_bus_feed")
        res = (out,) + ((tap_out,) if tap_out is not None else ()) + ((aux_out,) if aux_out is not None else ())
        return res[0] if len(res) == 1 else res

    def process_block_bus_feed_dev(self, d_src, d_out, n_samples, group=1, mix_out=False, stream=None, d_tap_out=None, d_aux_out=None):
        """The same with pointers the device can address (ints or contiguous float32 torch tensors); single-shard handles;
        asynchronous on `stream`.  A d_src in device memory is gathered in place, anything else is copied to the device first."""
        def ptr(t):
            return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        return self._check(self._lib.fxb_process_block_bus_feed_dev(self._h, ptr(d_src), ptr(d_out), ptr(d_tap_out), ptr(d_aux_out), int(n_samples), int(group),
                                                                     BUS_MIX_OUT if mix_out else 0, C.c_void_p(stream or 0)), "process_block_bus_feed_dev")

    def _stream_stride(self, shape, strides):
        """the instance stride (in floats) when an [N, S, channels] array is N interleaved [S][channels] runs at one stride, else None"""
        n, S, ch = shape
        if (n, ch) != (self.n, self.channels) or (ch > 1 and strides[2] != 1) or (S > 1 and strides[1] != ch):
            return None
        return S * ch if n == 1 else (strides[0] if strides[0] >= S * ch else None)

    def process_block_imajor(self, x, out=None):
        """A block of per-instance streams.  x: float32 [N, S, channels] - instance n's interleaved [S][channels] run - returns the
        same shape (into `out` when given).  A view with unit inner strides and one instance stride, e.g. whole[:, f0:f0 + S, :] of
        a pinned [N, frames, channels] array, goes to the library as it is, with its stride: in place when the memory is pinned.
        Other layouts are copied."""
        def stride(a):
            ok = isinstance(a, np.ndarray) and a.dtype == np.float32 and a.ndim == 3 and all(t % 4 == 0 for t in a.strides)
            return self._stream_stride(a.shape, [t // 4 for t in a.strides]) if ok else None
        if stride(x) is None:
            x = np.ascontiguousarray(x, dtype=np.float32)
            assert x.ndim == 3 and x.shape[0] == self.n and x.shape[2] == self.channels, "input must be [N, S, channels]"
        S = x.shape[1]
        given = out
        if out is None or stride(out) is None or not out.flags["WRITEABLE"] or out.shape != x.shape:
            out = np.empty((self.n, S, self.channels), dtype=np.float32)
        self._check(self._lib.fxb_process_block_imajor(self._h, C.c_void_p(x.ctypes.data), C.c_void_p(out.ctypes.data), S, stride(x), stride(out)), "process_block_imajor")
        if given is not None and given is not out:
            given[...] = out
            return given
        return out

    def process_block_imajor_dev(self, d_in, d_out, n_samples, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: device pointers (ints) with strides in floats (None: packed), or float32 torch tensors [N, n_samples,
        channels] whose inner strides are those of an interleaved run (views into a longer [N, frames, channels] tensor included;
        the instance stride comes from stride()).  Single-shard handles; asynchronous on `stream` (a hipStream_t as int)."""
        def ptr(t, given):
            if isinstance(t, int):
                return t, int(given or 0)
            assert t.element_size() == 4 and t.dim() == 3 and tuple(t.shape) == (self.n, n_samples, self.channels), "[N, S, channels] float32"
            st = self._stream_stride(tuple(t.shape), tuple(t.stride()))
            assert st is not None and given in (None, st), "N interleaved runs at one stride"
            return t.data_ptr(), st
        (a, sa), (b, sb) = ptr(d_in, in_stride), ptr(d_out, out_stride)
        return self._check(self._lib.fxb_process_block_imajor_dev(self._h, C.c_void_p(a), C.c_void_p(b), int(n_samples), sa, sb, C.c_void_p(stream or 0)),
                           "process_block_imajor_dev")

    def meter_enable(self, on=True):
        """Output meters on (accumulator rows allocated and zeroed on every shard; on twice keeps the values) or off (freed).
        While they are on, every launch of the program is followed by a small kernel that meters the block it wrote."""
        return self._check(self._lib.fxb_meter_enable(self._h, 1 if on else 0), "meter_enable")

    def meter_read(self, reset=False):
        """{"energy": float64, "peak": float32, "full_scale": uint32, "nonfinite": uint32}, each [channels, N] by global instance:
        what has accumulated since the last reset (include/fx8010_amd.h "Output meters").  Synchronous; reset: zero afterwards."""
        shape = (self.channels, self.n)
        out = {"energy": np.empty(shape, dtype=np.float64), "peak": np.empty(shape, dtype=np.float32),
               "full_scale": np.empty(shape, dtype=np.uint32), "nonfinite": np.empty(shape, dtype=np.uint32)}
        self._check(self._lib.fxb_meter_read(self._h, *[C.c_void_p(out[k].ctypes.data) for k in ("energy", "peak", "full_scale", "nonfinite")],
                                             1 if reset else 0), "meter_read")
        return out

    def meter_select(self, stat, threshold, below=False, first=0, n_range=None, cap=None):
        """(list, M): the global instance numbers in first .. first + n_range - 1 whose meter `stat` (METER_ENERGY, METER_PEAK,
        METER_FULL_SCALE, METER_NONFINITE), taken as the maximum over the channels, is >= threshold - with below: < threshold -
        compacted on the device into an ascending int64 list (include/fx8010_amd.h "Meter queries by list").  M is the number of
        matches; the list holds the min(M, cap) smallest.  n_range None: up to the last instance; cap None: n_range; cap 0 is a
        count query.  Exact: no rounding anywhere.  Synchronous; changes nothing."""
        first = int(first)
        n_range = self.n - first if n_range is None else int(n_range)
        cap = n_range if cap is None else int(cap)
        out = np.empty(max(min(cap, n_range), 0), dtype=np.int64)
        m = self._check(int(self._lib.fxb_meter_select(self._h, int(stat), float(threshold), first, n_range, C.c_void_p(out.ctypes.data) if out.size else None,
                                                       cap, METER_BELOW if below else 0)), "meter_select")
        return out[:min(m, out.size)], m

    def meter_read_list(self, instances, reset=False):
        """meter_read for the listed global instances only: {"energy", "peak", "full_scale", "nonfinite"}, each [channels,
        len(instances)], column k for instances[k], bit for bit what meter_read holds there - gathered on the device.  Synchronous.
        reset: the listed columns are zero afterwards, in the lane that read them (no instance may then be listed twice)."""
        lst = self._instance_list(instances)
        shape = (self.channels, lst.size)
        out = {"energy": np.zeros(shape, dtype=np.float64), "peak": np.zeros(shape, dtype=np.float32),
               "full_scale": np.zeros(shape, dtype=np.uint32), "nonfinite": np.zeros(shape, dtype=np.uint32)}
        self._check(self._lib.fxb_meter_read_list(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size),
                                                  *[C.c_void_p(out[k].ctypes.data) if lst.size else None for k in ("energy", "peak", "full_scale", "nonfinite")],
                                                  1 if reset else 0), "meter_read_list")
        return out

    def meter_reset_list(self, instances):
        """Zero the meters of the listed global instances only - a slot reused at note-on.  Stream-ordered behind the queued blocks
        and in front of later ones - it does not wait for them; sync(), meter_read, meter_read_list and meter_select cover it.
        meter_samples() stays the handle-wide count since the last full reset."""
        lst = self._instance_list(instances)
        return self._check(self._lib.fxb_meter_reset_list(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size)), "meter_reset_list")

    def meter_set_target(self, target, group=1, loop=False):
        """Set the target of the meters: `target` is [n_samples, channels, G] float32 with G = ceil(N / group); instance n is
        compared with column n // group (include/fx8010_amd.h "Target meters").  From now on the meter launch of every block also
        accumulates, per channel and instance, the squared error against the target and the cross product with it.  Synchronous;
        the position starts at 0.  loop: the target repeats; without it samples past its end change neither figure."""
        group = int(group)
        t = np.ascontiguousarray(target, dtype=np.float32)
        g = -(-self.n // min(max(group, 1), self.n))
        if t.ndim != 3 or t.shape[1:] != (self.channels, g):
            raise ValueError("meter_set_target: target must be [n_samples, %d, %d]" % (self.channels, g))
        return self._check(self._lib.fxb_meter_set_target(self._h, C.c_void_p(t.ctypes.data), int(t.shape[0]), group, METER_TARGET_LOOP if loop else 0), "meter_set_target")

    def meter_clear_target(self):
        """Drop the target: the target block and the two match rows are freed; the four meters go on."""
        return self._check(self._lib.fxb_meter_clear_target(self._h), "meter_clear_target")

    def meter_target_seek(self, pos):
        """the target position of the next queued block (host-side, no wait)"""
        return self._check(self._lib.fxb_meter_target_seek(self._h, int(pos)), "meter_target_seek")

    def meter_target_pos(self):
        """the target position the next queued block starts at"""
        return self._check(int(self._lib.fxb_meter_target_pos(self._h)), "meter_target_pos")

    def meter_read_match(self, reset=False):
        """{"err": float64, "cross": float64}, each [channels, N] by global instance: the squared error against the target and the
        cross product with it, accumulated since the last reset.  Synchronous; reset zeroes these two rows only."""
        shape = (self.channels, self.n)
        out = {"err": np.empty(shape, dtype=np.float64), "cross": np.empty(shape, dtype=np.float64)}
        self._check(self._lib.fxb_meter_read_match(self._h, C.c_void_p(out["err"].ctypes.data), C.c_void_p(out["cross"].ctypes.data), 1 if reset else 0), "meter_read_match")
        return out

    def meter_select_match(self, stat, threshold, below=False, first=0, n_range=None, cap=None):
        """meter_select over the match figures: V is the SUM over the channels of `stat` (MATCH_ERROR, MATCH_CROSS).  (list, M)."""
        first = int(first)
        n_range = self.n - first if n_range is None else int(n_range)
        cap = n_range if cap is None else int(cap)
        out = np.empty(max(min(cap, n_range), 0), dtype=np.int64)
        m = self._check(int(self._lib.fxb_meter_select_match(self._h, int(stat), float(threshold), first, n_range, C.c_void_p(out.ctypes.data) if out.size else None,
                                                             cap, METER_BELOW if below else 0)), "meter_select_match")
        return out[:min(m, out.size)], m

    def meter_best(self, stat=MATCH_ERROR, group=None, largest=False):
        """(winner int64 [G], value float64 [G]) with G = ceil(N / group): per group of `group` consecutive instances (None: all of
        them) the instance whose V - the channel sum of `stat` - is the smallest (largest: the largest), ties to the smallest
        number, and that V.  Found on the device; 16 bytes per group come back.  Synchronous."""
        group = self.n if group is None else int(group)
        g = -(-self.n // min(max(group, 1), self.n))
        winner, value = np.full(g, -1, dtype=np.int64), np.zeros(g, dtype=np.float64)
        self._check(self._lib.fxb_meter_best(self._h, int(stat), group, C.c_void_p(winner.ctypes.data), C.c_void_p(value.ctypes.data), MATCH_LARGEST if largest else 0), "meter_best")
        return winner, value

    def meter_set_level(self, release, floor=0.0):
        """Turn the level meters on (include/fx8010_amd.h "Level meters"): from now on the meter launch of every block also keeps,
        per channel and instance, an envelope - level = max(|y|, level * release) per sample - and the count of consecutive samples
        with |y| < floor.  0 <= release <= 1 (from a time constant: np.float32(np.exp(-1 / (tau * rate)))), floor >= 0.  The first
        call waits as sync() does and allocates; a call while the mode is on changes the parameters of later blocks only."""
        return self._check(self._lib.fxb_meter_set_level(self._h, float(release), float(floor), 0), "meter_set_level")

    def meter_clear_level(self):
        """Turn the level meters off: the two rows are freed; the other meters go on."""
        return self._check(self._lib.fxb_meter_clear_level(self._h), "meter_clear_level")

    def meter_get_level(self):
        """(release, floor) in force; an error while the level meters are off"""
        release, floor = C.c_float(0.0), C.c_float(0.0)
        self._check(self._lib.fxb_meter_get_level(self._h, C.byref(release), C.byref(floor)), "meter_get_level")
        return release.value, floor.value

    def meter_read_level(self, reset=False):
        """{"level": float32, "quiet": uint32}, each [channels, N] by global instance.  Synchronous; reset zeroes these two rows only."""
        shape = (self.channels, self.n)
        out = {"level": np.empty(shape, dtype=np.float32), "quiet": np.empty(shape, dtype=np.uint32)}
        self._check(self._lib.fxb_meter_read_level(self._h, C.c_void_p(out["level"].ctypes.data), C.c_void_p(out["quiet"].ctypes.data), 1 if reset else 0), "meter_read_level")
        return out

    def meter_read_level_list(self, instances, reset=False):
        """{"level", "quiet"}, each [channels, len(instances)]: the level meters of the listed instances, gathered on the device.
        An instance may repeat unless reset is set."""
        lst = self._instance_list(instances)
        shape = (self.channels, int(lst.size))
        out = {"level": np.empty(shape, dtype=np.float32), "quiet": np.empty(shape, dtype=np.uint32)}
        self._check(self._lib.fxb_meter_read_level_list(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size),
                                                        C.c_void_p(out["level"].ctypes.data) if lst.size else None, C.c_void_p(out["quiet"].ctypes.data) if lst.size else None,
                                                        1 if reset else 0), "meter_read_level_list")
        return out

    def meter_select_level(self, stat, threshold, below=False, first=0, n_range=None, cap=None):
        """meter_select over the level meters: V is the maximum over the channels of the envelope (LEVEL_ENVELOPE) or the MINIMUM
        over the channels of the quiet run (LEVEL_QUIET).  (list, M)."""
        first = int(first)
        n_range = self.n - first if n_range is None else int(n_range)
        cap = n_range if cap is None else int(cap)
        out = np.empty(max(min(cap, n_range), 0), dtype=np.int64)
        m = self._check(int(self._lib.fxb_meter_select_level(self._h, int(stat), float(threshold), first, n_range, C.c_void_p(out.ctypes.data) if out.size else None,
                                                             cap, METER_BELOW if below else 0)), "meter_select_level")
        return out[:min(m, out.size)], m

    def _meter_rank(self, name, stat, k, threshold, below, largest, first, n_range):
        first, k = int(first), int(k)
        n_range = self.n - first if n_range is None else int(n_range)
        room = max(min(k, n_range), 0)
        lst, val = np.empty(max(room, 1), dtype=np.int64), np.empty(max(room, 1), dtype=np.float64)   # (never null: k > 0 over an empty range is no refusal)
        m = self._check(int(getattr(self._lib, "fxb_" + name)(self._h, int(stat), k, float(threshold), first, n_range, C.c_void_p(lst.ctypes.data),
                                                              C.c_void_p(val.ctypes.data), (METER_BELOW if below else 0) | (METER_LARGEST if largest else 0))), name)
        r = min(m, room)
        return m, lst[:r], val[:r]

    def meter_rank(self, stat, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
        """The first k instances of first .. first + n_range - 1 under the order (V, n) - V as meter_select takes it, ascending (with
        `largest` descending), ties to the smaller instance number - among those meter_select would match (V >= threshold, with
        `below` V < threshold; the default takes the whole range), chosen on the device.  (M, list, values): M candidates, the
        min(M, k) instance numbers in rank order and their V."""
        return self._meter_rank("meter_rank", stat, k, threshold, below, largest, first, n_range)

    def meter_rank_match(self, stat, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
        """meter_rank over the match rows of a target: V is the channel sum of MATCH_ERROR or MATCH_CROSS.  (M, list, values)."""
        return self._meter_rank("meter_rank_match", stat, k, threshold, below, largest, first, n_range)

    def meter_rank_level(self, stat, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
        """meter_rank over the level meters: V is the channel maximum of the envelope (LEVEL_ENVELOPE) or the channel MINIMUM of the
        quiet run (LEVEL_QUIET) - the k quietest voices are meter_rank_level(LEVEL_ENVELOPE, k).  (M, list, values)."""
        return self._meter_rank("meter_rank_level", stat, k, threshold, below, largest, first, n_range)

    def meter_set_tones(self, coeff):
        """Turn the tone meters on (include/fx8010_amd.h "Tone meters"): from now on every block's meter launch is followed by a
        Goertzel recurrence per (tone, channel, instance) - s0 = (y + c * s1) - s2 in fp64, nothing fused - for the 1 .. 8
        coefficients given, each c = 2 * cos(2 * pi * f / fs) with -2 <= c <= 2.  Every call waits as sync() does and takes the
        rows into force zeroed."""
        c = np.ascontiguousarray(coeff, dtype=np.float64).reshape(-1)
        return self._check(self._lib.fxb_meter_set_tones(self._h, int(c.size), C.c_void_p(c.ctypes.data) if c.size else None, 0), "meter_set_tones")

    def meter_clear_tones(self):
        """Turn the tone meters off: the rows are freed; the other meters go on."""
        return self._check(self._lib.fxb_meter_clear_tones(self._h), "meter_clear_tones")

    def meter_get_tones(self):
        """the coefficients in force, float64 [K]; an error while the tone meters are off"""
        n, c = C.c_int(0), np.zeros(METER_MAX_TONES, dtype=np.float64)
        self._check(self._lib.fxb_meter_get_tones(self._h, C.byref(n), C.c_void_p(c.ctypes.data)), "meter_get_tones")
        return c[:n.value].copy()

    def _tone_rows(self, width):
        shape = (int(self.meter_get_tones().size), self.channels, width)
        return {k: np.empty(shape, dtype=np.float64) for k in ("s1", "s2", "power")}

    def meter_read_tones(self, reset=False):
        """{"s1", "s2", "power"}, each float64 [K, channels, N] by global instance: the two words of every recurrence and
        P = (s1*s1 + s2*s2) - (c*s1)*s2, about (A * n / 2) ** 2 after n samples of a sine of amplitude A at the probed bin.
        Synchronous; reset zeroes the tone rows only."""
        out = self._tone_rows(self.n)
        self._check(self._lib.fxb_meter_read_tones(self._h, C.c_void_p(out["s1"].ctypes.data), C.c_void_p(out["s2"].ctypes.data), C.c_void_p(out["power"].ctypes.data), 1 if reset else 0), "meter_read_tones")
        return out

    def meter_read_tones_list(self, instances, reset=False):
        """{"s1", "s2", "power"}, each [K, channels, len(instances)]: the tone meters of the listed instances, gathered on the
        device.  An instance may repeat unless reset is set."""
        lst = self._instance_list(instances)
        out = self._tone_rows(int(lst.size))
        ptrs = [C.c_void_p(out[k].ctypes.data) if lst.size else None for k in ("s1", "s2", "power")]
        self._check(self._lib.fxb_meter_read_tones_list(self._h, C.c_void_p(lst.ctypes.data) if lst.size else None, int(lst.size), ptrs[0], ptrs[1], ptrs[2], 1 if reset else 0), "meter_read_tones_list")
        return out

    def meter_select_tone(self, tone, threshold, below=False, first=0, n_range=None, cap=None):
        """meter_select over the tone meters: V is the maximum over the channels of the power at `tone`.  (list, M)."""
        first = int(first)
        n_range = self.n - first if n_range is None else int(n_range)
        cap = n_range if cap is None else int(cap)
        out = np.empty(max(min(cap, n_range), 0), dtype=np.int64)
        m = self._check(int(self._lib.fxb_meter_select_tone(self._h, int(tone), float(threshold), first, n_range, C.c_void_p(out.ctypes.data) if out.size else None,
                                                            cap, METER_BELOW if below else 0)), "meter_select_tone")
        return out[:min(m, out.size)], m

    def meter_rank_tone(self, tone, k, threshold=-np.inf, below=False, largest=False, first=0, n_range=None):
        """meter_rank over the tone meters: V is the maximum over the channels of the power at `tone` - the k voices that ring
        loudest at a pitch are meter_rank_tone(tone, k, largest=True).  (M, list, values)."""
        return self._meter_rank("meter_rank_tone", tone, k, threshold, below, largest, first, n_range)

    def meter_samples(self):
        """sample periods metered since the last reset"""
        return self._check(int(self._lib.fxb_meter_samples(self._h)), "meter_samples")

    def sync(self):
        return self._check(self._lib.fxb_sync(self._h), "sync")

    def instruction_counter(self):
        return int(self._lib.fxb_instruction_counter(self._h))

    def instruction_counter_i(self, inst):
        return int(self._lib.fxb_instruction_counter_i(self._h, inst))

    def ood_flags(self):
        return int(self._lib.fxb_ood_flags(self._h))

    def tier_note(self):
        """which tier runs the program as it stands, and why not a faster one"""
        buf = C.create_string_buffer(512)
        self._check(min(self._lib.fxb_tier_note(self._h, buf, 512), 0), "tier_note")
        return buf.value.decode("latin-1")

    def last_kernel_ms(self):
        return float(self._lib.fxb_last_kernel_ms(self._h))

    def info(self, what):
        return int(self._lib.fxb_info(self._h, INFO[what]))

    def last_error(self):
        return self._lib.fxb_last_error(self._h).decode("latin-1")


class Single(_Reports):
    """One emulated DSP with the reference's call-per-sample surface (fx_*)."""
    _pfx = "fx_"

    def __init__(self, channels=1):
        self._lib = load()
        self.channels = channels
        self._h = self._lib.fx_create(channels)
        if not self._h:
            raise RuntimeError("fx_create failed: " + self._lib.fx_last_create_error().decode("latin-1"))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fx_destroy(self._h)
            self._h = None

    __del__ = close

    def load_file(self, path):
        return bool(self._lib.fx_load_file(self._h, path.encode()))

    def process(self, sample):
        x = np.ascontiguousarray(sample, dtype=np.float32).reshape(self.channels)
        out = np.empty_like(x)
        rc = self._lib.fx_process(self._h, x.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
        if rc < 0:
            raise RuntimeError("fx_process failed: " + self._lib.fx_last_error(self._h).decode("latin-1"))
        return out

    def process_block(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty_like(x)
        rc = self._lib.fx_process_block(self._h, x.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p), x.size // self.channels)
        if rc < 0:
            raise RuntimeError("fx_process_block failed: " + self._lib.fx_last_error(self._h).decode("latin-1"))
        return out

    def set_register(self, key, v):
        return int(self._lib.fx_set_register(self._h, key.encode(), C.c_float(v)))

    def get_register(self, key):
        return float(self._lib.fx_get_register(self._h, key.encode()))

    def instruction_counter(self):
        return int(self._lib.fx_instruction_counter(self._h))
