"""CPU: the entry points of sharded proofs with H in evaluation form (include/zkr.h zkr_key_shard_opts,
zkr_prove_sharded_last_h_form) check their arguments before any device call, and the shards' counts of unsatisfied rows
(csrc/shard_group.hpp ShardGroup::unsatisfied) add up over host threads."""
import ctypes
import os
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.environ.get("ZKR_HOSTARITH_LIB") or os.path.join(ROOT, "simple-zk-rollups_amd", "csrc", "libzkr_hostarith.so")


def test_both_symbols_are_exported_and_bound():
    import zkr_hip
    L = zkr_hip.lib()
    assert hasattr(L, "zkr_key_shard_opts") and hasattr(L, "zkr_prove_sharded_last_h_form")
    assert zkr_hip.binding.SHARD_SIDE_TABLES == 1 and callable(zkr_hip.sharded_last_h_form)


def test_shard_opts_refuses_null_pointers_and_unknown_flags_without_a_device():
    import zkr_hip
    L = zkr_hip.lib()
    out = ctypes.c_void_p()
    assert L.zkr_key_shard_opts(None, 0, 2, 0, 0, ctypes.byref(out)) == -5 and b"null" in L.zkr_last_error()
    assert L.zkr_key_shard_opts(None, 0, 2, 0, 1, ctypes.byref(out)) == -5
    # the flags are looked at before the key is: a buffer of zeros stands in for one
    not_a_key = ctypes.create_string_buffer(1 << 16)
    assert L.zkr_key_shard_opts(ctypes.cast(not_a_key, ctypes.c_void_p), 0, 2, 0, 0x2, ctypes.byref(out)) == -5
    assert b"unknown flags 0x2" in L.zkr_last_error()
    assert L.zkr_key_shard_opts(ctypes.cast(not_a_key, ctypes.c_void_p), 0, 2, 0, 0x3, ctypes.byref(out)) == -5
    assert L.zkr_key_shard_opts(ctypes.cast(not_a_key, ctypes.c_void_p), 0, 2, 0, 1, None) == -5 and b"null" in L.zkr_last_error()
    assert not out.value


def test_last_h_form_is_none_on_a_fresh_thread():
    import zkr_hip
    L = zkr_hip.lib()
    assert L.zkr_prove_sharded_last_h_form(None, None, 0) == -5
    seen = {}

    def fresh():
        form, buf = ctypes.c_int(7), ctypes.create_string_buffer(b"x" * 7, 8)
        seen["rc"] = L.zkr_prove_sharded_last_h_form(ctypes.byref(form), buf, 8)
        seen["form"], seen["reason"] = form.value, buf.value
        seen["binding"] = zkr_hip.sharded_last_h_form()

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert seen == {"rc": 0, "form": 0, "reason": b"", "binding": {"form": "none", "reason": ""}}


def test_shard_group_sums_the_counts_of_eight_threads():
    S = ctypes.CDLL(SHIM)
    S.zkr_host_shard_group_count_selftest.restype = ctypes.c_ulonglong
    S.zkr_host_shard_group_count_selftest.argtypes = [ctypes.c_uint, ctypes.POINTER(ctypes.c_uint)]
    for counts in ([0] * 8, [0, 0, 0, 0, 0, 0, 0, 1], [3, 1, 4, 1, 5, 9, 2, 6], [0xffffffff] * 8):
        assert S.zkr_host_shard_group_count_selftest(8, (ctypes.c_uint * 8)(*counts)) == sum(counts)  # past 2^32: the sum is 64 bits wide
    assert S.zkr_host_shard_group_count_selftest(1, (ctypes.c_uint * 1)(7)) == 7
