"""ctypes binding of libzkr_hip.so (declarations follow include/zkr.h one to one)."""
import collections
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZKR_HIP_LIB") or os.path.normpath(os.path.join(_HERE, "..", "..", "csrc", "libzkr_hip.so"))  # same override as index.js
PROOF_BYTES = 256
PARTIAL_BYTES = 640   # zkr.h ZKR_PARTIAL_BYTES
SHARD_SIDE_TABLES = 1  # ZKR_SHARD_SIDE_TABLES
EXPORT_STANDARD = 1  # ZKR_EXPORT_STANDARD
CONTRIBUTION_BYTES = 352   # zkr.h ZKR_CONTRIBUTION_BYTES
KeyAudit = collections.namedtuple("KeyAudit", "valid step detail phase1_contributions delta_contributions")   # ProvingKey.audit
PTAU_RECORD_BYTES = 928   # zkr.h ZKR_PTAU_RECORD_BYTES
REPLICATE_MODES = {"auto": 0, "full": 1, "base": 2}   # zkr.h ZKR_REPLICATE_*
KEY_SECTIONS = ("none", "rowptr", "col", "wide", "rank", "header", "points", "twiddles", "coef", "shared rank", "consts")   # zkr.h ZKR_KEYSEC_*
STAGES = ("ingest", "spmv", "ntt", "msm_sort", "msm_accum_g1", "msm_accum_g2", "msm_big", "msm_reduce", "total",
          "spmv_a", "ntt_pass", "combine_h")   # the last three: single streaming kernels (bench.py roofline.streaming)
_lib = None


class BookOpts(ctypes.Structure):   # zkr.h zkr_book_opts
    _fields_ = [("nullifier_cap_log2", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("salt", ctypes.c_uint64)]


class OperatorOpts(ctypes.Structure):   # zkr.h zkr_operator_opts
    _fields_ = [("batch", ctypes.c_uint32), ("max_batches", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class KeyExportOpts(ctypes.Structure):   # zkr.h zkr_key_export_opts
    _fields_ = [("flags", ctypes.c_uint32), ("piece_points", ctypes.c_uint32)]


class WprogOpts(ctypes.Structure):   # zkr.h zkr_wprog_opts
    _fields_ = [("piece", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class NttSelftestDesc(ctypes.Structure):   # zkr.h zkr_ntt_selftest_desc
    _fields_ = [(f, ctypes.c_uint32) for f in ("logn", "tlog", "dif", "inverse", "pre", "nbat", "pair", "in_place", "want_lo", "want_n", "coset_shift",
                                               "coset_add", "cross", "klog", "col_lo", "col_n", "in_sub", "out_sub", "canon", "reserved")]


class ZkrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("zkr error %d: %s" % (code, msg))
        self.code = code


def lib():
    """Load the HIP library; fail loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZkrError(-1, "HIP extension %s is missing: run __graft_entry__.build() "
                           "(make -C simple-zk-rollups_amd/csrc); there is no CPU fallback" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    c = ctypes
    vp, sz, u8p, i = c.c_void_p, c.c_size_t, c.c_char_p, c.c_int
    L.zkr_last_error.restype = c.c_char_p
    L.zkr_version.restype = c.c_char_p
    L.zkr_device_count.restype = i
    L.zkr_device_pci_bus_id.argtypes = [i, c.c_char_p, sz]
    L.zkr_key_load_websnark.argtypes = [u8p, sz, i, c.POINTER(vp)]
    L.zkr_key_free.argtypes = [vp]
    L.zkr_key_free.restype = None
    L.zkr_key_info.argtypes = [vp, c.POINTER(c.c_uint64)]
    L.zkr_key_save.argtypes = [vp, c.c_char_p]
    L.zkr_key_load_file.argtypes = [c.c_char_p, i, c.POINTER(vp)]
    L.zkr_key_slots.argtypes = [vp]
    L.zkr_key_fuse.argtypes = [vp]
    L.zkr_prove_batch_device.argtypes = [vp, c.POINTER(vp), sz, u8p, u8p, vp, u8p]
    L.zkr_key_windows.argtypes = [vp, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    L.zkr_key_arena.argtypes = [vp, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_key_adopt_arena.argtypes = [vp, sz, i, c.POINTER(vp)]
    L.zkr_key_base_arena.argtypes = [vp, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_key_adopt_base_arena.argtypes = [vp, sz, i, c.POINTER(vp)]
    L.zkr_key_check.argtypes = [vp, i, c.POINTER(c.c_uint64)]
    L.zkr_r1cs_load.argtypes = [u8p, sz, i, c.POINTER(vp)]
    L.zkr_r1cs_free.argtypes = [vp]
    L.zkr_r1cs_free.restype = None
    L.zkr_r1cs_info.argtypes = [vp, c.POINTER(c.c_uint64)]
    L.zkr_r1cs_check_device.argtypes = [vp, c.POINTER(vp), sz, vp, c.POINTER(c.c_uint64), c.POINTER(i)]
    L.zkr_r1cs_check.argtypes = [vp, c.POINTER(c.c_char_p), sz, sz, c.POINTER(c.c_uint64), c.POINTER(i)]
    L.zkr_r1cs_matches_key.argtypes = [vp, vp, c.POINTER(i)]
    L.zkr_wprog_load.argtypes = [u8p, sz, i, c.POINTER(vp)]
    L.zkr_wprog_load_opts.argtypes = [u8p, sz, i, c.POINTER(WprogOpts), c.POINTER(vp)]
    L.zkr_wprog_free.argtypes = [vp]
    L.zkr_wprog_free.restype = None
    L.zkr_wprog_info.argtypes = [vp, c.POINTER(c.c_uint64)]
    L.zkr_wprog_shape.argtypes = [u8p, sz, c.POINTER(c.c_uint64)]
    L.zkr_wprog_witness_batch_device.argtypes = [vp, vp, sz, vp, c.POINTER(c.c_uint32), vp]
    L.zkr_wprog_witness_batch.argtypes = [vp, u8p, sz, vp, c.POINTER(c.c_uint32)]
    L.zkr_wprog_stage_times.argtypes = [vp, c.POINTER(c.c_double)]
    L.zkr_wprog_run_host.argtypes = [u8p, sz, u8p, u8p, u8p, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    L.zkr_mimcsponge_round_constants.argtypes = [u8p]
    L.zkr_key_replicate.argtypes = [vp, i, i, c.POINTER(vp)]
    L.zkr_key_contribute.argtypes = [vp, u8p, c.POINTER(vp), u8p]
    L.zkr_contribution_check.argtypes = [u8p, c.POINTER(i)]
    L.zkr_key_contribution_verify.argtypes = [vp, vp, u8p, c.POINTER(i), c.POINTER(c.c_uint64)]
    L.zkr_vk_contribute.argtypes = [u8p, sz, u8p, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_contribution_chain_check.argtypes = [u8p, sz, c.POINTER(i)]
    L.zkr_key_audit.argtypes = [vp, vp, u8p, sz, u8p, sz, u8p, sz, u8p, sz, c.POINTER(i), c.POINTER(c.c_uint64)]
    L.zkr_ptau_new.argtypes = [c.c_uint, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_ptau_contribute.argtypes = [u8p, sz, u8p, i, c.POINTER(vp), c.POINTER(sz), u8p]
    L.zkr_ptau_record_check.argtypes = [u8p, sz, c.POINTER(i)]
    L.zkr_ptau_verify.argtypes = [u8p, sz, u8p, sz, i, c.POINTER(i), c.POINTER(c.c_uint64)]
    L.zkr_setup_r1cs_ptau.argtypes = [u8p, sz, u8p, sz, i, c.POINTER(vp), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_points_scale_each.argtypes = [u8p, u8p, sz, i, i]
    L.zkr_group_ntt.argtypes = [u8p, c.c_uint, i, i, i]
    L.zkr_key_device.argtypes = [vp]
    L.zkr_key_replication.argtypes = [vp, c.POINTER(i), c.POINTER(i)]
    L.zkr_prove_sharded_last_form.argtypes = [c.POINTER(i), c.c_char_p, sz]
    L.zkr_prove_batch_multi.argtypes = [c.POINTER(vp), sz, c.POINTER(c.c_char_p), sz, sz, u8p, u8p, u8p]
    L.zkr_prove_batch_multi_device.argtypes = [c.POINTER(vp), sz, c.POINTER(vp), sz, u8p, u8p, u8p]
    L.zkr_key_shard.argtypes = [vp, c.c_uint, c.c_uint, i, c.POINTER(vp)]
    L.zkr_key_shard_opts.argtypes = [vp, c.c_uint, c.c_uint, i, c.c_uint, c.POINTER(vp)]
    L.zkr_prove_sharded_last_h_form.argtypes = [c.POINTER(i), c.c_char_p, sz]
    L.zkr_key_shard_info.argtypes = [vp, c.POINTER(c.c_uint32)]
    L.zkr_prove_partial.argtypes = [vp, u8p, sz, u8p]
    L.zkr_prove_partial_device.argtypes = [vp, vp, vp, u8p]
    L.zkr_prove_combine.argtypes = [vp, u8p, sz, u8p, u8p, u8p]
    L.zkr_prove_sharded.argtypes = [c.POINTER(vp), sz, u8p, sz, u8p, u8p, u8p]
    L.zkr_prove_sharded_device.argtypes = [c.POINTER(vp), sz, c.POINTER(vp), u8p, u8p, u8p]
    L.zkr_prove.argtypes = [vp, u8p, sz, u8p, u8p, u8p, vp]
    L.zkr_prove_device.argtypes = [vp, vp, u8p, u8p, u8p, vp]
    L.zkr_prove_submit.argtypes = [vp, vp, u8p, u8p, vp, c.POINTER(i)]
    L.zkr_prove_collect.argtypes = [vp, i, u8p]
    L.zkr_prove_batch.argtypes = [vp, c.POINTER(c.c_char_p), sz, sz, u8p, u8p, u8p]
    L.zkr_verify.argtypes = [u8p, sz, u8p, u8p, sz, c.POINTER(i)]
    L.zkr_verify_batch.argtypes = [u8p, sz, u8p, u8p, sz, sz, c.POINTER(i)]
    L.zkr_vk_load.argtypes = [u8p, sz, i, c.POINTER(vp)]
    L.zkr_vk_free.argtypes = [vp]
    L.zkr_vk_free.restype = None
    L.zkr_vk_info.argtypes = [vp, c.POINTER(c.c_uint64)]
    L.zkr_verify_each.argtypes = [vp, u8p, u8p, sz, vp, c.POINTER(i)]
    L.zkr_verify_each_device.argtypes = [vp, u8p, c.POINTER(vp), sz, vp, vp, c.POINTER(i)]
    L.zkr_pairing_device.argtypes = [u8p, u8p, sz, vp, vp, i]
    L.zkr_ntt.argtypes = [u8p, c.c_uint, i, i]
    L.zkr_msm_g1.argtypes = [u8p, u8p, sz, u8p, c.POINTER(i), i]
    L.zkr_msm_g2.argtypes = [u8p, u8p, sz, u8p, c.POINTER(i), i]
    L.zkr_calc_h.argtypes = [vp, u8p, sz, u8p]
    L.zkr_prof_enable.argtypes = [vp, i]
    L.zkr_prof_reset.argtypes = [vp]
    L.zkr_prof_get.argtypes = [vp, c.c_char_p, c.POINTER(c.c_double), c.POINTER(c.c_uint64)]
    L.zkr_synth_key.argtypes = [c.c_uint, c.c_uint, c.c_uint64, c.c_uint64, i, c.POINTER(vp), c.POINTER(vp), c.POINTER(sz),
                                c.POINTER(vp), c.POINTER(sz)]
    L.zkr_synth_websnark.argtypes = [c.c_uint, c.c_uint, c.c_uint64, c.c_uint64, i, c.POINTER(vp), c.POINTER(sz),
                                     c.POINTER(vp), c.POINTER(sz)]
    L.zkr_synth_witness.argtypes = [c.c_uint, c.c_uint, c.c_uint64, c.c_uint64, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_setup_r1cs.argtypes = [u8p, sz, u8p, i, c.POINTER(vp), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_setup_r1cs_opts.argtypes = [u8p, sz, u8p, i, c.c_uint, c.POINTER(vp), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_key_h_form.argtypes = [vp, c.POINTER(i), c.POINTER(c.c_uint64)]
    L.zkr_key_eval_tables.argtypes = [vp, u8p, sz, c.c_uint, c.POINTER(i)]
    L.zkr_key_eval_tables_drop.argtypes = [vp]
    L.zkr_key_eval_tables_equal.argtypes = [vp, vp, c.POINTER(i)]
    L.zkr_points_add_each.argtypes = [u8p, u8p, sz, i, i]
    L.zkr_setup_r1cs_websnark.argtypes = [u8p, sz, u8p, i, c.POINTER(vp), c.POINTER(sz), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_key_export_websnark.argtypes = [vp, c.POINTER(KeyExportOpts), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_key_export_last_times.argtypes = [c.POINTER(c.c_double)]
    L.zkr_websnark_len.argtypes = [c.c_uint64] * 5 + [c.POINTER(c.c_uint64)]
    L.zkr_websnark_render_host.argtypes = [c.c_uint32, c.c_uint32, c.c_uint32, u8p, vp, vp, u8p, vp, vp, u8p, c.POINTER(c.c_char_p), c.POINTER(vp), c.POINTER(sz)]
    L.zkr_synth_vk.argtypes = [vp, u8p, sz, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_synth_set_shape.argtypes = [c.c_uint]
    L.zkr_free.argtypes = [vp]
    L.zkr_free.restype = None
    L.zkr_bench_fq_mul.argtypes = [i, c.POINTER(c.c_double)]
    L.zkr_bench_fq_mul_legacy.argtypes = [i, c.POINTER(c.c_double)]
    L.zkr_selftest_f29_forms.argtypes = [i, i, i, c.POINTER(c.c_uint32), sz, c.POINTER(c.c_uint32)]
    L.zkr_selftest_curve29.argtypes = [i, i, i, c.POINTER(c.c_uint32), sz, c.POINTER(c.c_uint32), c.POINTER(c.c_uint8)]
    L.zkr_selftest_fp.argtypes = [i, i, i, c.POINTER(c.c_uint32), sz, c.POINTER(c.c_uint32)]
    L.zkr_selftest_ntt.argtypes = [i, c.POINTER(NttSelftestDesc)] + [vp] * 6
    L.zkr_mimcsponge_multihash.argtypes = [u8p, sz, u8p]
    L.zkr_babyjub_pubkey.argtypes = [u8p, u8p]
    L.zkr_eddsa_sign.argtypes = [u8p, u8p, sz, u8p]
    L.zkr_eddsa_verify.argtypes = [u8p, sz, u8p, u8p, c.POINTER(i)]
    L.zkr_mimcsponge_multihash_batch.argtypes = [u8p, sz, c.c_uint, u8p, i]
    L.zkr_balance_tree_build.argtypes = [u8p, c.c_uint, u8p, i]
    L.zkr_babyjub_format_privkey.argtypes = [u8p, u8p]
    L.zkr_withdraw_r1cs.argtypes = [c.POINTER(vp), c.POINTER(sz)]
    L.zkr_withdraw_witness.argtypes = [u8p, u8p, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_rollup_info.argtypes = [c.c_uint32, c.c_uint32, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    L.zkr_rollup_r1cs.argtypes = [c.c_uint32, c.c_uint32, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_rollup_witness.argtypes = [c.c_uint32, c.c_uint32, u8p, sz, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_rollup_witness_batch_device.argtypes = [c.c_uint32, c.c_uint32, u8p, sz, sz, vp, c.c_int]
    L.zkr_rollup_witness_program_host.argtypes = [c.c_uint32, c.c_uint32, u8p, sz, vp, c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    L.zkr_rollup_statement_text.argtypes = [c.c_uint32]
    L.zkr_rollup_statement_text.restype = c.c_char_p
    L.zkr_rollup_witness_batch_from_device.argtypes = [c.c_uint32, c.c_uint32, vp, sz, sz, vp, c.c_int, vp]
    L.zkr_babyjub_format_privkey_batch.argtypes = [u8p, sz, u8p, i]
    L.zkr_babyjub_pubkey_batch.argtypes = [u8p, sz, u8p, i]
    L.zkr_eddsa_sign_batch.argtypes = [u8p, u8p, c.c_uint, sz, u8p, i]
    L.zkr_withdraw_witness_batch_device.argtypes = [u8p, u8p, sz, vp, i, vp]
    L.zkr_wallet_pubkey_program_host.argtypes = [u8p, u8p, u8p]
    L.zkr_wallet_sign_program_host.argtypes = [u8p, u8p, c.c_uint, u8p]
    L.zkr_withdraw_witness_program_host.argtypes = [u8p, u8p, vp, c.POINTER(c.c_uint32)]
    L.zkr_withdraw_statement_text.argtypes = [c.c_uint32]
    L.zkr_withdraw_statement_text.restype = c.c_char_p
    L.zkr_withdraw_n_vars.argtypes = []
    L.zkr_mimc7_round_constants.argtypes = [u8p]
    L.zkr_mimc7_hash.argtypes = [u8p, u8p, u8p]
    L.zkr_mimc7_multihash.argtypes = [u8p, sz, u8p, u8p]
    L.zkr_babyjub_ecdh.argtypes = [u8p, u8p, u8p]
    L.zkr_mimc7_encrypt.argtypes = [u8p, u8p, c.c_uint, u8p, u8p]
    L.zkr_mimc7_decrypt.argtypes = [u8p, u8p, u8p, c.c_uint, u8p]
    L.zkr_babyjub_ecdh_batch.argtypes = [u8p, u8p, sz, u8p, i]
    L.zkr_mimc7_encrypt_batch.argtypes = [u8p, u8p, c.c_uint, sz, u8p, u8p, i]
    L.zkr_mimc7_decrypt_batch.argtypes = [u8p, u8p, u8p, c.c_uint, sz, u8p, i]
    L.zkr_ecdh_encrypt_batch.argtypes = [u8p, u8p, u8p, c.c_uint, sz, u8p, u8p, i]
    L.zkr_ecdh_decrypt_batch.argtypes = [u8p, u8p, u8p, u8p, c.c_uint, sz, u8p, i]
    L.zkr_withdraw_n_vars.restype = c.c_uint32
    L.zkr_ledger_new.argtypes = [c.c_uint, i, c.POINTER(vp)]
    L.zkr_ledger_free.argtypes = [vp]
    L.zkr_ledger_free.restype = None
    L.zkr_ledger_deposit.argtypes = [vp, c.POINTER(c.c_uint32), u8p, sz]
    L.zkr_ledger_info.argtypes = [vp, c.POINTER(c.c_uint64)]
    L.zkr_ledger_root.argtypes = [vp, u8p]
    L.zkr_ledger_account.argtypes = [vp, c.c_uint32, u8p, u8p]
    L.zkr_ledger_sequence.argtypes = [vp, u8p, sz, c.c_uint32, u8p, vp, c.POINTER(sz), c.POINTER(sz), vp]
    L.zkr_ledger_stage_times.argtypes = [vp, c.POINTER(c.c_double)]
    L.zkr_eddsa_verify_batch.argtypes = [u8p, c.c_uint, u8p, u8p, sz, u8p, i]
    L.zkr_sequence_plan_host.argtypes = [c.c_uint, u8p, sz, u8p, sz, u8p, c.c_uint32, u8p, c.POINTER(sz), c.POINTER(c.c_int32)]
    L.zkr_ledger_replay.argtypes = [vp, u8p, sz, c.c_uint32, u8p, c.c_uint32, u8p, c.POINTER(c.c_uint32), c.POINTER(sz), vp]
    L.zkr_ledger_replay_device.argtypes = [vp, c.POINTER(vp), sz, c.c_uint32, u8p, c.c_uint32, u8p, c.POINTER(c.c_uint32), c.POINTER(sz), vp]
    L.zkr_replay_plan_host.argtypes = [c.c_uint, u8p, sz, u8p, sz, c.c_uint32, u8p, c.POINTER(c.c_uint32), c.POINTER(sz), c.POINTER(c.c_uint32), u8p, u8p,
                                       c.POINTER(c.c_int32)]
    u64p = c.POINTER(c.c_uint64)
    L.zkr_ledger_records.argtypes = [vp, sz, sz, u8p]
    L.zkr_ledger_tree.argtypes = [vp, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_ledger_snapshot.argtypes = [vp, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_ledger_save.argtypes = [vp, c.c_char_p]
    L.zkr_ledger_snapshot_check.argtypes = [u8p, sz, u64p, c.POINTER(c.c_int)]
    L.zkr_ledger_restore.argtypes = [u8p, sz, i, c.POINTER(vp)]
    L.zkr_ledger_load_file.argtypes = [c.c_char_p, i, c.POINTER(vp)]
    L.zkr_ledger_checkpoint.argtypes = [vp, u64p]
    L.zkr_ledger_rollback.argtypes = [vp, c.c_uint64]
    L.zkr_ledger_release.argtypes = [vp, c.c_uint64]
    L.zkr_ledger_journal_info.argtypes = [vp, u64p]
    L.zkr_ledger_audit.argtypes = [vp, u64p, c.POINTER(c.c_int)]
    u32p = c.POINTER(c.c_uint32)
    L.zkr_ledger_book_open.argtypes = [vp, c.POINTER(BookOpts), u8p, sz]
    L.zkr_ledger_book_info.argtypes = [vp, u64p]
    L.zkr_ledger_deposit_calls.argtypes = [vp, u8p, u8p, sz, u8p, u32p, u8p]
    L.zkr_ledger_withdraw_calls.argtypes = [vp, u8p, u8p, u8p, sz, u8p, u32p, u8p]
    L.zkr_ledger_withdraw_calls_device.argtypes = [vp, c.POINTER(vp), u8p, u8p, sz, u8p, u32p, u8p, vp]
    L.zkr_ledger_lookup_keys.argtypes = [vp, u8p, sz, u32p]
    L.zkr_ledger_nullifiers_used.argtypes = [vp, u8p, sz, u8p]
    L.zkr_ledger_fees.argtypes = [vp, u8p, i]
    L.zkr_ledger_book_blob.argtypes = [vp, c.POINTER(vp), c.POINTER(sz)]
    L.zkr_book_blob_check.argtypes = [u8p, sz, u64p, c.POINTER(c.c_int)]
    L.zkr_book_deposit_plan_host.argtypes = [c.c_uint, u8p, sz, u8p, u8p, sz, u32p, u8p, u32p, u8p]
    L.zkr_book_withdraw_plan_host.argtypes = [u8p, sz, u8p, u8p, u8p, sz, u32p, u8p, u32p, u8p]
    L.zkr_operator_new.argtypes = [vp, vp, vp, vp, c.POINTER(OperatorOpts), c.POINTER(vp)]
    L.zkr_operator_free.argtypes = [vp]
    L.zkr_operator_free.restype = None
    L.zkr_operator_info.argtypes = [vp, u64p]
    L.zkr_operator_step.argtypes = [vp, u8p, sz, u8p, u8p, u8p, u8p, vp, c.POINTER(sz), c.POINTER(sz)]
    L.zkr_operator_stage_times.argtypes = [vp, c.POINTER(c.c_double)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise ZkrError(rc, lib().zkr_last_error().decode())


def device_count():
    return lib().zkr_device_count()


def device_pci_bus_id(device=0) -> str:
    buf = ctypes.create_string_buffer(32)
    _check(lib().zkr_device_pci_bus_id(device, buf, 32))
    return buf.value.decode()


def version():
    return lib().zkr_version().decode()


def websnark_len(n_vars, n_public, domain, nnz_a, nnz_b) -> int:
    """Length of a websnark proving key with these sizes (zkr_websnark_len, host only); ZkrError -5 past the format's 2^32 - 1."""
    out = ctypes.c_uint64()
    _check(lib().zkr_websnark_len(n_vars, n_public, domain, nnz_a, nnz_b, ctypes.byref(out)))
    return int(out.value)


def websnark_render_host(n_vars, n_public, domain, consts448, side_a, side_b, points) -> bytes:
    """The websnark bytes from their parts (zkr_websnark_render_host, host only).  side_a / side_b: (rowptr, col, coefs) of a QAP
    side in CSR by row -- two lists of ints and the coefficients as 32-byte strings end to end; points: the five sections A, B1,
    B2, C, hExps as bytes."""
    import struct
    def side(sd):
        rowptr, col, coef = sd
        return struct.pack("<%dI" % len(rowptr), *rowptr), struct.pack("<%dI" % len(col), *col), bytes(coef)
    ra, ca, fa = side(side_a)
    rb, cb, fb = side(side_b)
    pts = (ctypes.c_char_p * 5)(*[bytes(x) for x in points])
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib().zkr_websnark_render_host(n_vars, n_public, domain, bytes(consts448), ra, ca, fa, rb, cb, fb, pts, ctypes.byref(out), ctypes.byref(n)))
    return _take(out, n.value)


def json_key_from_standard(buf: bytes) -> dict:
    """The snarkjs JSON proving key from the standard-form export (ProvingKey.to_standard)."""
    import struct
    R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    n, p, m = struct.unpack_from("<3I", buf, 0)
    ptr = struct.unpack_from("<7I", buf, 12)
    num = lambda o: str(int.from_bytes(buf[o:o + 32], "little"))

    def g1(o):
        x, y = num(o), num(o + 32)
        return [x, y, "0" if x == "0" else "1"]

    def g2(o):
        x, y = [num(o), num(o + 32)], [num(o + 64), num(o + 96)]
        return [x, y, ["0", "0"] if x == ["0", "0"] else ["1", "0"]]

    def pols(o):
        out = []
        for _ in range(n):
            (k,) = struct.unpack_from("<I", buf, o)
            o += 4
            d = {}
            for _ in range(k):
                (c,) = struct.unpack_from("<I", buf, o)
                v = int.from_bytes(buf[o + 4:o + 36], "little")
                d[c] = (d[c] + v) % R if c in d else v
                o += 36
            out.append({str(c): str(v) for c, v in d.items()})
        return out

    return {"protocol": "groth", "nVars": n, "nPublic": p, "domainBits": m.bit_length() - 1, "domainSize": m,
            "polsA": pols(ptr[0]), "polsB": pols(ptr[1]),
            "A": [g1(ptr[2] + 64 * i) for i in range(n)], "B1": [g1(ptr[3] + 64 * i) for i in range(n)],
            "B2": [g2(ptr[4] + 128 * i) for i in range(n)],
            "C": [None] * (p + 1) + [g1(ptr[5] + 64 * i) for i in range(n - p - 1)],
            "hExps": [g1(ptr[6] + 64 * i) for i in range(m)],
            "vk_alfa_1": g1(40), "vk_beta_1": g1(104), "vk_delta_1": g1(168), "vk_beta_2": g2(232), "vk_delta_2": g2(360)}


def _take(ptr, n):
    data = ctypes.string_at(ptr, n)
    lib().zkr_free(ptr)
    return data


class ProvingKey:
    """Device-resident proving key (zkr_key*)."""

    def __init__(self, handle, device, keepalive=None):
        self._h = handle
        self.device = device
        self._keepalive = keepalive  # e.g. the torch tensor that owns an adopted arena

    @classmethod
    def load_websnark(cls, pk_bin: bytes, device=0):
        h = ctypes.c_void_p()
        _check(lib().zkr_key_load_websnark(bytes(pk_bin), len(pk_bin), device, ctypes.byref(h)))
        return cls(h, device)

    @classmethod
    def synth(cls, log_m, n_public=73, circuit_seed=0x5A4B0001, toxic_seed=0x5A4B00FF, device=0, want_aux=True):
        """-> (key, witness_bytes, aux_bytes_or_None); key points are computed on the GPU."""
        h, w, a = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        wl, al = ctypes.c_size_t(), ctypes.c_size_t()
        _check(lib().zkr_synth_key(log_m, n_public, circuit_seed, toxic_seed, device, ctypes.byref(h), ctypes.byref(w),
                                   ctypes.byref(wl), ctypes.byref(a) if want_aux else None,
                                   ctypes.byref(al) if want_aux else None))
        witness = _take(w, wl.value)
        aux = _take(a, al.value) if want_aux else None
        return cls(h, device), witness, aux

    @classmethod
    def adopt_arena(cls, dev_ptr, length, device, keepalive=None):
        h = ctypes.c_void_p()
        _check(lib().zkr_key_adopt_arena(ctypes.c_void_p(dev_ptr), length, device, ctypes.byref(h)))
        return cls(h, device, keepalive)

    @classmethod
    def adopt_base_arena(cls, dev_ptr, length, device):
        """Full key rebuilt on `device` from the compact arena bytes (zkr_key_adopt_base_arena); the buffer is not kept."""
        h = ctypes.c_void_p()
        _check(lib().zkr_key_adopt_base_arena(ctypes.c_void_p(dev_ptr), length, device, ctypes.byref(h)))
        return cls(h, device)

    @classmethod
    def setup_r1cs(cls, r1cs_bin: bytes, toxic=None, device=0, side_tables=True):
        """Groth16 setup of an R1CS on the GPU (zkr_setup_r1cs; `snarkjs setup --protocol groth`).  toxic: None (OS
        CSPRNG) or five ints (t, alfa, beta, gamma, delta) for reproducible tests.  side_tables=False refuses the allocation of
        the evaluation-form side tables (zkr_setup_r1cs_opts: a test hook for the fall-back).  Returns (key, vk_bin)."""
        tb = None if toxic is None else b"".join(int(x).to_bytes(32, "little") for x in toxic)
        h, vk, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        if side_tables:
            _check(lib().zkr_setup_r1cs(bytes(r1cs_bin), len(r1cs_bin), tb, device, ctypes.byref(h), ctypes.byref(vk), ctypes.byref(n)))
        else:
            _check(lib().zkr_setup_r1cs_opts(bytes(r1cs_bin), len(r1cs_bin), tb, device, 1, ctypes.byref(h), ctypes.byref(vk), ctypes.byref(n)))
        try:
            return cls(h, device), ctypes.string_at(vk, n.value)
        finally:
            lib().zkr_free(vk)

    @classmethod
    def setup_r1cs_ptau(cls, r1cs_bin: bytes, ptau: bytes, device=0):
        """Groth16 setup of an R1CS from a powers-of-tau transcript (zkr_setup_r1cs_ptau): nobody knows t, alfa, beta; delta =
        gamma = 1, so at least one contribute() must follow before the key guards anything.  Returns (key, vk_bin)."""
        h, vk, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_setup_r1cs_ptau(bytes(r1cs_bin), len(r1cs_bin), bytes(ptau), len(ptau), device, ctypes.byref(h), ctypes.byref(vk), ctypes.byref(n)))
        try:
            return cls(h, device), ctypes.string_at(vk, n.value)
        finally:
            lib().zkr_free(vk)

    @classmethod
    def load_file(cls, path, device=0):
        """Packed key written by save(): one read + one upload, no parse, no window-table rebuild."""
        h = ctypes.c_void_p()
        _check(lib().zkr_key_load_file(os.fsencode(path), device, ctypes.byref(h)))
        return cls(h, device)

    def check(self, level=0):
        """What the key's arena contains (zkr_key_check): level 0 the structure (every index a kernel follows stays inside its
        section), level 1 also the values (points on their curves at every window level, twiddles, coefficients below r, shared
        rank maps, header constants).  A clean key returns the report {"bad": 0, "section": "none", "part": 0, "first": 0};
        a damaged one raises ZkrError (code -2) naming the first faulty section."""
        rep = (ctypes.c_uint64 * 4)()
        _check(lib().zkr_key_check(self._h, level, rep))
        return {"bad": int(rep[0]), "section": KEY_SECTIONS[rep[1]], "part": int(rep[2]), "first": int(rep[3])}

    def save(self, path):
        _check(lib().zkr_key_save(self._h, os.fsencode(path)))

    def replicate(self, device, mode="auto"):
        """An independent replica of this key on `device` (zkr_key_replicate): device-to-device copy inside this process,
        no torch.distributed.  mode "full" (whole arena, adopted as is), "base" (compact arena + rebuild of the window
        levels) or "auto" (full when the devices address each other).  `device` may be the key's own."""
        h = ctypes.c_void_p()
        _check(lib().zkr_key_replicate(self._h, device, REPLICATE_MODES[mode], ctypes.byref(h)))
        return ProvingKey(h, device)

    def contribute(self, d=None):
        """A further party's delta contribution (zkr_key_contribute): -> (new ProvingKey on the same device, the 352-byte
        record).  d: None (drawn from the OS CSPRNG inside the call and wiped there) or an int with 1 < d < r for reproducible
        tests.  This key stays as it is, so the pair can be verified."""
        db = None if d is None else int(d).to_bytes(32, "little")
        h = ctypes.c_void_p()
        rec = ctypes.create_string_buffer(CONTRIBUTION_BYTES)
        _check(lib().zkr_key_contribute(self._h, db, ctypes.byref(h), ctypes.cast(rec, ctypes.c_char_p)))
        return ProvingKey(h, self.device), rec.raw

    def contribution_verify(self, after, record: bytes):
        """What a party that did not make the contribution runs (zkr_key_contribution_verify): self = the key before, `after` the
        key it was handed -> (valid, first failed step or 0, ZKR_KEYSEC_* number of the first differing section for steps 3 and 4:
        KEY_SECTIONS names it)."""
        assert len(record) == CONTRIBUTION_BYTES
        ok = ctypes.c_int(0)
        rep = (ctypes.c_uint64 * 2)()
        _check(lib().zkr_key_contribution_verify(self._h, after._h, bytes(record), ctypes.byref(ok), rep))
        return bool(ok.value), int(rep[0]), int(rep[1])

    def audit(self, system, ptau, ptau_records=(), delta_records=(), vk_bin=b""):
        """What somebody who took no part in the ceremony runs on the finished key (zkr_key_audit): are this proving key and
        `vk_bin` the ones `system` (a ConstraintSystem on this key's device) and the transcript `ptau` give, with delta moved only by the
        contributors of `delta_records`?  Records: lists of records or their concatenation, in the order they were made.
        -> KeyAudit(valid, step, detail, phase1_contributions, delta_contributions); step = the first failed step (0: none),
        detail = the record's index (step 3) or the table (steps 5 and 6: 0 A, 1 B1, 2 B2, 3 C, 4 hExps; 5: the twiddles);
        zkr_hip.lib().zkr_last_error() names what failed.  A key with delta_contributions == 0 is consistent and NOT sound."""
        pr, dr = _records(ptau_records, PTAU_RECORD_BYTES), _records(delta_records, CONTRIBUTION_BYTES)
        ok = ctypes.c_int(0)
        rep = (ctypes.c_uint64 * 4)()
        _check(lib().zkr_key_audit(self._h, system._h, bytes(ptau), len(ptau), pr if pr else None, len(pr) // PTAU_RECORD_BYTES, dr if dr else None,
                                   len(dr) // CONTRIBUTION_BYTES, bytes(vk_bin), len(vk_bin), ctypes.byref(ok), rep))
        return KeyAudit(bool(ok.value), int(rep[0]), int(rep[1]), int(rep[2]), int(rep[3]))

    def replication(self):
        """How this key came to its device (zkr_key_replication): {"mode": "none" | "full" | "base", "peer_direct": bool}."""
        mode, direct = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().zkr_key_replication(self._h, ctypes.byref(mode), ctypes.byref(direct)))
        return {"mode": {0: "none", 1: "full", 2: "base"}[mode.value], "peer_direct": bool(direct.value)}

    def shard(self, part, parts, device=None, side_tables=False):
        """Shard `part` of `parts` of this (whole) key on `device` (default: the key's own): the points of one contiguous range
        of every MSM of a proof, all window levels, plus the whole QAP (zkr_key_shard).
        side_tables: also the shard's range of the side tables of the evaluation form, when this key has them
        (zkr_key_shard_opts with ZKR_SHARD_SIDE_TABLES): prove_sharded over shards that ALL have them runs H in evaluation
        form.  A shard that could not get them is a coefficient-form shard (h_form() says so, zkr_last_error() why)."""
        h = ctypes.c_void_p()
        dev = self.device if device is None else device
        _check(lib().zkr_key_shard_opts(self._h, part, parts, dev, SHARD_SIDE_TABLES if side_tables else 0, ctypes.byref(h)))
        return ProvingKey(h, dev)

    def bench_split_solo(self, d_witness_ptr) -> float:
        """Measurement only: this shard's share of a proof with a split calcH, alone, own buffers standing in for the other
        shards' (zkr_bench_shard_split_solo) -> milliseconds.  The result of the computation is meaningless and discarded."""
        ms = ctypes.c_double(0)
        _check(lib().zkr_bench_shard_split_solo(self._h, ctypes.c_void_p(d_witness_ptr), ctypes.byref(ms)))
        return ms.value

    def shard_info(self):
        out = (ctypes.c_uint32 * 6)()
        _check(lib().zkr_key_shard_info(self._h, out))
        return dict(zip(("part", "parts", "w_lo", "w_n", "h_lo", "h_n"), [int(x) for x in out]))

    def prove_partial(self, witness: bytes) -> bytes:
        """This shard's partial sums of A, B1, B2, C + H for one proof (zkr_prove_partial), PARTIAL_BYTES opaque bytes."""
        out = ctypes.create_string_buffer(PARTIAL_BYTES)
        _check(lib().zkr_prove_partial(self._h, bytes(witness), len(witness), out))
        return out.raw

    def prove_partial_device(self, d_witness_ptr, stream=None) -> bytes:
        out = ctypes.create_string_buffer(PARTIAL_BYTES)
        _check(lib().zkr_prove_partial_device(self._h, ctypes.c_void_p(d_witness_ptr), ctypes.c_void_p(stream or 0), out))
        return out.raw

    def prove_combine(self, partials, r=None, s=None) -> bytes:
        """The proof from the partial sums of all shards (zkr_prove_combine); self: any shard or the whole key."""
        out = ctypes.create_string_buffer(PROOF_BYTES)
        rb = None if r is None else int(r).to_bytes(32, "little")
        sb = None if s is None else int(s).to_bytes(32, "little")
        _check(lib().zkr_prove_combine(self._h, b"".join(partials), len(partials), rb, sb, out))
        return out.raw

    def close(self):
        if self._h:
            lib().zkr_key_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        out = (ctypes.c_uint64 * 10)()
        _check(lib().zkr_key_info(self._h, out))
        names = ("nVars", "nPublic", "domainSize", "nnzA", "nnzB", "ptsA", "ptsB1", "ptsB2", "ptsC", "ptsH")
        return dict(zip(names, [int(x) for x in out]))

    def h_form(self):
        """How this key's own proofs form the H term -- not part of info(), which describes the arena and is equal for a key and
        its replicas, while the side tables of the evaluation form stay with the key that was built with them.  {'form': 'evaluation' | 'coefficients', 'retries': witnesses proved again through the coefficient form because they
        left constraints unsatisfied -- lone proofs and fused groups alike; a group goes again as a whole and counts the witnesses
        that failed} (zkr_key_h_form)."""
        ev, n = ctypes.c_int(), ctypes.c_uint64()
        _check(lib().zkr_key_h_form(self._h, ctypes.byref(ev), ctypes.byref(n)))
        return {"form": "evaluation" if ev.value else "coefficients", "retries": int(n.value)}

    def eval_tables(self, r1cs_bin: bytes) -> bool:
        """The side tables of the evaluation form from this key's own points and the circuit's C side (zkr_key_eval_tables): any
        whole key -- websnark bytes, a file, a transcript, a replica, a contributed key.  True: h_form() says 'evaluation' from
        now on.  False: the key keeps the coefficient form and zkr_hip.lib().zkr_last_error() says why.  Saving, replicating
        and contributing carry no tables: derive again on the key they return; shard(side_tables=True) cuts them with the shard."""
        built = ctypes.c_int(0)
        _check(lib().zkr_key_eval_tables(self._h, bytes(r1cs_bin), len(r1cs_bin), 0, ctypes.byref(built)))
        return bool(built.value)

    def drop_eval_tables(self):
        """Back to the coefficient form; frees the side tables (zkr_key_eval_tables_drop)."""
        _check(lib().zkr_key_eval_tables_drop(self._h))

    def eval_tables_equal(self, other) -> bool:
        """Both keys have side tables and they are equal byte for byte (zkr_key_eval_tables_equal, a test hook)."""
        same = ctypes.c_int(0)
        _check(lib().zkr_key_eval_tables_equal(self._h, other._h, ctypes.byref(same)))
        return bool(same.value)

    def arena(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_key_arena(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def base_arena(self):
        """(device pointer, length) of the compact arena: base points + QAP rows, no window levels (zkr_key_base_arena)."""
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_key_base_arena(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def _export(self, flags, piece_points):
        opts = KeyExportOpts(flags, int(piece_points or 0))
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_key_export_websnark(self._h, ctypes.byref(opts), ctypes.byref(out), ctypes.byref(n)))
        return _take(out, n.value)

    def to_websnark(self, piece_points=None) -> bytes:
        """This key as the provingKeyBin `binarifyProvingKey` writes (zkr_key_export_websnark): what load_websnark reads, what the
        reference's groth16GenProof and the checkers take.  Any whole key: loaded, adopted, replicated, set up from scalars or
        from a transcript, contributed.  piece_points: output points per table handled at a time (default 2^20)."""
        return self._export(0, piece_points)

    def to_standard(self, piece_points=None) -> bytes:
        """The same layout with every field element in standard form (ZKR_EXPORT_STANDARD): what to_json_key() reads."""
        return self._export(EXPORT_STANDARD, piece_points)

    @staticmethod
    def export_times():
        """The calling thread's last export (zkr_key_export_last_times): milliseconds by part and the extra device bytes held."""
        out = (ctypes.c_double * 5)()
        _check(lib().zkr_key_export_last_times(out))
        return {"kernels_ms": out[0], "copies_ms": out[1], "host_ms": out[2], "total_ms": out[3], "device_bytes": int(out[4])}

    def to_json_key(self) -> dict:
        """This key in the snarkjs 0.1.20 JSON shape binarify.ts:129-138,152-202 reads (the reference's `*_pk.json`): decimal
        strings, points as [x, y, "1"] (infinity ["0", "1", "0"]), C None for the public signals, polsA / polsB one
        {constraint: coefficient} object per signal.  An object holds one coefficient per constraint: terms a key stores twice
        for one (signal, constraint) are added."""
        return json_key_from_standard(self.to_standard())

    def prove(self, witness: bytes, r=None, s=None, stream=None) -> bytes:
        out = ctypes.create_string_buffer(PROOF_BYTES)
        rb = None if r is None else int(r).to_bytes(32, "little")
        sb = None if s is None else int(s).to_bytes(32, "little")
        _check(lib().zkr_prove(self._h, bytes(witness), len(witness), rb, sb, out, ctypes.c_void_p(stream or 0)))
        return out.raw

    def prove_device(self, d_witness_ptr, r=None, s=None, stream=None) -> bytes:
        out = ctypes.create_string_buffer(PROOF_BYTES)
        rb = None if r is None else int(r).to_bytes(32, "little")
        sb = None if s is None else int(s).to_bytes(32, "little")
        _check(lib().zkr_prove_device(self._h, ctypes.c_void_p(d_witness_ptr), rb, sb, out, ctypes.c_void_p(stream or 0)))
        return out.raw

    def synth_vk(self, aux: bytes) -> bytes:
        """vk_bin (zkr_verify layout) of a key made by ProvingKey.synth, from its checker blob."""
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().zkr_synth_vk(self._h, bytes(aux), len(aux), ctypes.byref(out), ctypes.byref(n)))
        try:
            return ctypes.string_at(out, n.value)
        finally:
            lib().zkr_free(out)

    def windows(self):
        """{table: (window bits c, windows K)} for A, B1, B2, C, H."""
        cs, ks = (ctypes.c_uint32 * 5)(), (ctypes.c_uint32 * 5)()
        _check(lib().zkr_key_windows(self._h, cs, ks))
        return {t: (cs[i], ks[i]) for i, t in enumerate(("A", "B1", "B2", "C", "H"))}

    def prove_submit(self, d_witness_ptr, r=None, s=None, stream=None) -> int:
        """Enqueue the GPU side of one proof, return a ticket (zkr_prove_submit); at most two in flight."""
        rb = None if r is None else int(r).to_bytes(32, "little")
        sb = None if s is None else int(s).to_bytes(32, "little")
        ticket = ctypes.c_int(-1)
        _check(lib().zkr_prove_submit(self._h, ctypes.c_void_p(d_witness_ptr), rb, sb, ctypes.c_void_p(stream or 0), ctypes.byref(ticket)))
        return ticket.value

    def prove_collect(self, ticket) -> bytes:
        out = ctypes.create_string_buffer(PROOF_BYTES)
        _check(lib().zkr_prove_collect(self._h, int(ticket), out))
        return out.raw

    def prove_batch_device(self, d_witness_ptrs, rs=None, ss=None, stream=None, depth=None):
        """Independent proofs of one batch from witnesses resident in HBM (zkr_prove_batch_device): two submits in flight,
        proofs of small circuits fused into shared launches (fuse() per submit), in the four-transform form when the key has the side
        tables (h_form()).  depth (or env ZKR_PIPELINE_DEPTH) selects
        the unfused submit / collect loop with that many single proofs in flight instead."""
        import collections
        import os
        depth = depth or int(os.environ.get("ZKR_PIPELINE_DEPTH", "0"))
        n = len(d_witness_ptrs)
        if not depth:
            if n == 0:
                return []
            arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p) for p in d_witness_ptrs])
            rb, sb = _blinding_bytes(rs, ss, n)
            out = ctypes.create_string_buffer(256 * n)
            _check(lib().zkr_prove_batch_device(self._h, arr, n, rb, sb, ctypes.c_void_p(stream or 0), out))
            return [out.raw[256 * i:256 * i + 256] for i in range(n)]
        out, pending = [], collections.deque()
        for j, ptr in enumerate(d_witness_ptrs):
            if len(pending) == depth:
                out.append(self.prove_collect(pending.popleft()))
            pending.append(self.prove_submit(ptr, None if rs is None else rs[j], None if ss is None else ss[j], stream))
        while pending:
            out.append(self.prove_collect(pending.popleft()))
        return out

    def prove_batch(self, witnesses, rs=None, ss=None):
        """zkr_prove_batch: host witnesses (bytes, equal length) -> list of 256-byte proofs, uploads and proofs pipelined."""
        n = len(witnesses)
        if n == 0:
            return []
        wlen = _equal_length(witnesses)
        arr = (ctypes.c_char_p * n)(*[bytes(w) for w in witnesses])
        rb, sb = _blinding_bytes(rs, ss, n)
        out = ctypes.create_string_buffer(256 * n)
        _check(lib().zkr_prove_batch(self._h, arr, wlen, n, rb, sb, out))
        return [out.raw[256 * i:256 * i + 256] for i in range(n)]

    def slots(self):
        """Submits the key can hold in flight (zkr_prove_submit before zkr_prove_collect)."""
        return lib().zkr_key_slots(self._h)

    def fuse(self):
        """Proofs one batch submit runs in shared launches (zkr_key_fuse): 1 for circuits that fill the chip alone."""
        return lib().zkr_key_fuse(self._h)

    def calc_h(self, witness: bytes) -> bytes:
        m = self.info()["domainSize"]
        out = ctypes.create_string_buffer(32 * m)
        _check(lib().zkr_calc_h(self._h, bytes(witness), len(witness), out))
        return out.raw

    def prof_enable(self, on=True):
        _check(lib().zkr_prof_enable(self._h, 1 if on else 0))

    def prof_reset(self):
        _check(lib().zkr_prof_reset(self._h))

    def prof(self):
        """{stage: (ms_total, launches)} measured with hipEvents on the launch stream."""
        out = {}
        for st in STAGES:
            ms, n = ctypes.c_double(), ctypes.c_uint64()
            _check(lib().zkr_prof_get(self._h, st.encode(), ctypes.byref(ms), ctypes.byref(n)))
            out[st] = (ms.value, n.value)
        return out


class ConstraintSystem:
    """A rank-1 constraint system resident on the device (zkr_r1cs*): does a witness satisfy it, and if not, which constraint
    fails first -- before the proof, where ProvingKey.prove* would return a proof no verifier accepts.  One ConstraintSystem
    serves one call at a time."""

    def __init__(self, handle, device):
        self._h = handle
        self.device = device

    @classmethod
    def load(cls, r1cs_bin: bytes, device=0):
        """r1cs_bin as ProvingKey.setup_r1cs takes it (binarify_r1cs, RollupCircuit.r1cs)."""
        h = ctypes.c_void_p()
        _check(lib().zkr_r1cs_load(bytes(r1cs_bin), len(r1cs_bin), device, ctypes.byref(h)))
        return cls(h, device)

    def info(self):
        out = (ctypes.c_uint64 * 6)()
        _check(lib().zkr_r1cs_info(self._h, out))
        return dict(zip(("nVars", "nPublic", "nConstraints", "nnzA", "nnzB", "nnzC"), [int(x) for x in out]))

    @staticmethod
    def _reports(rep, n):
        none = (1 << 64) - 1
        return [{"violated": int(rep[3 * j]), "first": None if rep[3 * j + 1] == none else int(rep[3 * j + 1]), "one_ok": rep[3 * j + 2] == 0} for j in range(n)]

    def check(self, witnesses):
        """zkr_r1cs_check: host witnesses (bytes of equal length, nVars x 32 B standard form) -> (all satisfied, one report per
        witness: {"violated": count, "first": smallest violated constraint or None, "one_ok": signal 0 is 1}).  A violated witness
        raises nothing; zkr_hip.lib().zkr_last_error() names the first one."""
        n = len(witnesses)
        if n == 0:
            raise ValueError("no witness to check")
        wlen = _equal_length(witnesses)
        arr = (ctypes.c_char_p * n)(*[bytes(w) for w in witnesses])
        rep = (ctypes.c_uint64 * (3 * n))()
        ok = ctypes.c_int(0)
        _check(lib().zkr_r1cs_check(self._h, arr, wlen, n, rep, ctypes.byref(ok)))
        return bool(ok.value), self._reports(rep, n)

    def check_device(self, d_witness_ptrs, stream=None):
        """zkr_r1cs_check_device: the same for witnesses resident in HBM on the system's device (device pointers, e.g.
        t[i].data_ptr() of RollupCircuit.calculate_witness_batch_device); stream as for ProvingKey.prove_device."""
        n = len(d_witness_ptrs)
        if n == 0:
            raise ValueError("no witness to check")
        arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p) for p in d_witness_ptrs])
        rep = (ctypes.c_uint64 * (3 * n))()
        ok = ctypes.c_int(0)
        _check(lib().zkr_r1cs_check_device(self._h, arr, n, ctypes.c_void_p(stream or 0), rep, ctypes.byref(ok)))
        return bool(ok.value), self._reports(rep, n)

    def matches_key(self, key) -> bool:
        """zkr_r1cs_matches_key: is `key` (a ProvingKey on the same device) a key of this system?  Binds the A and B sides only:
        a key has no C side, so a system that differs in C alone still matches."""
        same = ctypes.c_int(0)
        _check(lib().zkr_r1cs_matches_key(self._h, key._h, ctypes.byref(same)))
        return bool(same.value)

    def close(self):
        if self._h:
            lib().zkr_r1cs_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


WPROG_INFO = ("nInputs", "nWires", "nInstructions", "nVars", "nPublic", "workspaceBytes", "piece", "nStatements")   # zkr_wprog_info
WPROG_CODES = ("ok", "an input is not below r", "an assertion failed")   # reports[0] of zkr_wprog_witness_batch_device
WitnessRun = collections.namedtuple("WitnessRun", "code statement witness wires")   # WitnessProgram.run_host


def mimcsponge_round_constants():
    """The 220 round constants of multi_hash as integers (zkr_mimcsponge_round_constants, host only)."""
    out = ctypes.create_string_buffer(220 * 32)
    _check(lib().zkr_mimcsponge_round_constants(out))
    return [int.from_bytes(out.raw[32 * k:32 * k + 32], "little") for k in range(220)]


def wprog_shape(wprog_bin: bytes) -> dict:
    """Counts of a witness program from its bytes (zkr_wprog_shape: the validator, host only); ZkrError -5 names what is malformed."""
    out = (ctypes.c_uint64 * 8)()
    _check(lib().zkr_wprog_shape(bytes(wprog_bin), len(wprog_bin), out))
    return {k: int(v) for k, v in zip(WPROG_INFO, out) if k not in ("workspaceBytes", "piece")}


def wprog_run_host(wprog_bin: bytes, row, want_wires=False) -> WitnessRun:
    """zkr_wprog_run_host: ONE instance on the host through the interpreter step the kernel runs; no device.  row: n_inputs ints
    below 2^256.  -> WitnessRun(code, statement, witness bytes (n_vars x 32, zeros unless code == 0), wires bytes or None)."""
    shape = wprog_shape(wprog_bin)
    if len(row) != shape["nInputs"]:
        raise ValueError("the program takes %d inputs, got %d" % (shape["nInputs"], len(row)))
    ins = b"".join(int(v).to_bytes(32, "little") for v in row)
    wit = ctypes.create_string_buffer(32 * shape["nVars"])
    wires = ctypes.create_string_buffer(32 * shape["nWires"]) if want_wires else None
    code, stmt = ctypes.c_uint32(), ctypes.c_uint32()
    _check(lib().zkr_wprog_run_host(bytes(wprog_bin), len(wprog_bin), ins, wit, wires, ctypes.byref(code), ctypes.byref(stmt)))
    return WitnessRun(code.value, stmt.value, wit.raw, wires.raw if want_wires else None)


class WitnessProgram:
    """A witness program resident on the device (zkr_wprog*): witnesses of a whole batch of instances of ANY circuit, one GPU lane
    per instance, laid out as ProvingKey.prove_batch_device and ConstraintSystem.check_device take them.  wprog_bin comes from a
    front end (zkr_hip.circuit.Circuit.program()); statements: its statement texts, used in error messages.  piece: instances
    per pass over the wire store (None: the library's default).  One WitnessProgram serves one call at a time."""

    def __init__(self, wprog_bin: bytes, device=0, piece=None, statements=None):
        self._h = None
        self.bin = bytes(wprog_bin)
        self.statements = list(statements) if statements is not None else []
        self.device = device
        self.reports = []
        h = ctypes.c_void_p()
        opts = WprogOpts(int(piece or 0), 0)
        _check(lib().zkr_wprog_load_opts(self.bin, len(self.bin), device, ctypes.byref(opts), ctypes.byref(h)))
        self._h = h

    def info(self):
        out = (ctypes.c_uint64 * 8)()
        _check(lib().zkr_wprog_info(self._h, out))
        return dict(zip(WPROG_INFO, [int(x) for x in out]))

    def statement_text(self, stmt):
        return self.statements[stmt] if stmt < len(self.statements) else "statement %d" % stmt

    def _raise(self, err, reports):
        """The library's error with the failing instance's statement in the front end's words."""
        if err.code != -7:
            raise err
        j = next(k for k, r in enumerate(reports) if r[0])
        code, stmt = reports[j]
        what = "input %d is not below r" % stmt if code == 1 else "violates: %s" % self.statement_text(stmt)
        e = ZkrError(err.code, "instance %d %s" % (j, what))
        e.reports = reports
        raise e from None

    def witness_batch_device(self, inputs, stream=None):
        """zkr_wprog_witness_batch_device / zkr_wprog_witness_batch.  inputs: a torch.uint8 tensor on the program's device holding
        n x n_inputs x 32 B (standard form), or a list of rows of ints, which are checked against r on the host and uploaded.
        stream: the stream (a torch stream or a raw handle) the inputs were written on.  -> torch.uint8 [n, n_vars * 32] on the
        device; row j's data_ptr() is witness j.  self.reports: [(code, statement)] of the call.  An instance that fails raises
        ZkrError -7 naming the first one with its statement text; e.reports has every instance's, and the witnesses of the
        others are complete (self.last holds the tensor)."""
        import torch
        info = self.info()
        ni, nv = info["nInputs"], info["nVars"]
        dev = torch.device("cuda", self.device)
        raw = getattr(stream, "cuda_stream", stream) or 0
        if isinstance(inputs, torch.Tensor):
            if inputs.dtype != torch.uint8 or not inputs.is_cuda or inputs.device.index != self.device or not inputs.is_contiguous():
                raise ValueError("inputs must be a contiguous torch.uint8 tensor on cuda:%d" % self.device)
            if inputs.numel() % (32 * ni or 32):
                raise ValueError("inputs hold %d bytes, not a multiple of n_inputs x 32 = %d" % (inputs.numel(), 32 * ni))
            n = inputs.numel() // (32 * ni) if ni else int(inputs.shape[0])
            host = None
        else:
            rows = [list(r) for r in inputs]
            if any(len(r) != ni for r in rows):
                raise ValueError("every row must hold the program's %d inputs" % ni)
            n = len(rows)
            host = b"".join(int(v).to_bytes(32, "little") for r in rows for v in r)
        out = torch.empty((n, nv * 32), dtype=torch.uint8, device=dev)
        rep = (ctypes.c_uint32 * (2 * n or 1))()
        self.last = out
        try:
            if host is None:
                _check(lib().zkr_wprog_witness_batch_device(self._h, ctypes.c_void_p(inputs.data_ptr()), n, ctypes.c_void_p(out.data_ptr()), rep, ctypes.c_void_p(raw)))
            else:
                _check(lib().zkr_wprog_witness_batch(self._h, host, n, ctypes.c_void_p(out.data_ptr()), rep))
        except ZkrError as e:
            self.reports = [(int(rep[2 * j]), int(rep[2 * j + 1])) for j in range(n)]
            self._raise(e, self.reports)
        self.reports = [(int(rep[2 * j]), int(rep[2 * j + 1])) for j in range(n)]
        return out

    def stage_times(self):
        """Milliseconds of the last batch call in the interpreter kernel and in the layout kernel (zkr_wprog_stage_times)."""
        out = (ctypes.c_double * 2)()
        _check(lib().zkr_wprog_stage_times(self._h, out))
        return {"run_ms": out[0], "layout_ms": out[1]}

    def run_host(self, row, want_wires=False) -> WitnessRun:
        """One instance on the host (wprog_run_host); raises nothing for a failing instance: look at .code and .statement."""
        return wprog_run_host(self.bin, row, want_wires)

    def close(self):
        if self._h:
            lib().zkr_wprog_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


VERDICTS = ("valid", "bad G1 point", "public signal not below r", "bad G2 point", "pairing equation fails")   # zkr.h ZKR_VERDICT_*


class VerifyingKey:
    """A verifying key resident on the device (zkr_vk*): the Groth16 acceptance check with one verdict per proof (0 = valid,
    else the first failing check: VERDICTS).  vk_bin: the layout of zkr_hip.verify (binarify_verifying_key).  A failing proof
    raises nothing; zkr_hip.lib().zkr_last_error() names the first one, and .all_valid holds the call's *all_valid.  One VerifyingKey
    serves one call at a time."""

    def __init__(self, vk_bin: bytes, device=0):
        self._h = None
        h = ctypes.c_void_p()
        _check(lib().zkr_vk_load(bytes(vk_bin), len(vk_bin), device, ctypes.byref(h)))
        self._h = h
        self.device = device
        self.all_valid = None   # of the last verify_each* call
        out = (ctypes.c_uint64 * 2)()
        _check(lib().zkr_vk_info(self._h, out))
        self.n_public = int(out[0])

    def _proofs(self, proofs):
        pb = b"".join(bytes(p) for p in proofs)
        if len(pb) != PROOF_BYTES * len(proofs):
            raise ValueError("every proof is %d bytes" % PROOF_BYTES)
        return pb

    def verify_each(self, proofs, public_signals):
        """zkr_verify_each: proofs (256 B each) and one list of n_public ints per proof, both from the host -> one verdict per proof."""
        n = len(proofs)
        if len(public_signals) != n or any(len(p) != self.n_public for p in public_signals):
            raise ValueError("one list of %d public signals per proof" % self.n_public)
        sb = b"".join(int(v).to_bytes(32, "little") for p in public_signals for v in p)
        verdicts = ctypes.create_string_buffer(max(n, 1))
        ok = ctypes.c_int(0)
        _check(lib().zkr_verify_each(self._h, self._proofs(proofs), sb, n, verdicts, ctypes.byref(ok)))
        self.all_valid = bool(ok.value)
        return list(verdicts.raw[:n])

    def verify_each_device(self, proofs, d_witness_ptrs, stream=None):
        """zkr_verify_each_device: the public signals are words 1..n_public of the witnesses where they live (device pointers on
        the key's device, as ProvingKey.prove_batch_device takes them); stream as for ProvingKey.prove_device."""
        n = len(proofs)
        if len(d_witness_ptrs) != n:
            raise ValueError("one witness pointer per proof")
        arr = (ctypes.c_void_p * max(n, 1))(*[ctypes.c_void_p(p) for p in d_witness_ptrs])
        verdicts = ctypes.create_string_buffer(max(n, 1))
        ok = ctypes.c_int(0)
        _check(lib().zkr_verify_each_device(self._h, self._proofs(proofs), arr, n, ctypes.c_void_p(stream or 0), verdicts, ctypes.byref(ok)))
        self.all_valid = bool(ok.value)
        return list(verdicts.raw[:n])

    def close(self):
        if self._h:
            lib().zkr_vk_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pairing_device(g1: bytes, g2: bytes, device=0):
    """zkr_pairing_device: e(P_i, Q_i) for n pairs of standard-form affine points (64 B / 128 B each, all zero = infinity) ->
    (n x 384 B of Fq12 coefficients in the tower's order, n degenerate flags)."""
    n = len(g1) // 64
    if len(g1) != 64 * n or len(g2) != 128 * n:
        raise ValueError("g1 is n x 64 bytes and g2 n x 128 bytes")
    out = ctypes.create_string_buffer(max(384 * n, 1))
    deg = ctypes.create_string_buffer(max(n, 1))
    _check(lib().zkr_pairing_device(bytes(g1), bytes(g2), n, out, deg, device))
    return out.raw[:384 * n], list(deg.raw[:n])


def _blinding_bytes(rs, ss, n=None):
    """r / s of a batch as 32-byte LE records.  The C side reads 32 * count bytes of each: a short list must not reach it."""
    if (rs is None) != (ss is None):
        raise ValueError("pass both rs and ss or neither")
    if rs is not None and n is not None and (len(rs) != n or len(ss) != n):
        raise ValueError("a batch of %d proofs needs %d blinding scalars of each kind, got %d and %d" % (n, n, len(rs), len(ss)))
    rb = None if rs is None else b"".join(int(x).to_bytes(32, "little") for x in rs)
    sb = None if ss is None else b"".join(int(x).to_bytes(32, "little") for x in ss)
    return rb, sb


def _equal_length(witnesses):
    """The batch calls pass ONE witness_len for every pointer: a shorter buffer would be read past its end."""
    n0 = len(witnesses[0])
    for i, w in enumerate(witnesses):
        if len(w) != n0:
            raise ValueError("witness %d is %d bytes, witness 0 is %d: a batch takes witnesses of one circuit" % (i, len(w), n0))
    return n0


def prove_batch_multi(keys, witnesses, rs=None, ss=None):
    """zkr_prove_batch_multi: one batch of independent proofs over several replicas of a key (ProvingKey.replicate), proof i
    on keys[i mod len(keys)], one host thread per key inside the library.  witnesses: host bytes of equal length."""
    n = len(witnesses)
    if n == 0:
        return []
    ks = (ctypes.c_void_p * len(keys))(*[k._h for k in keys])
    wlen = _equal_length(witnesses)
    arr = (ctypes.c_char_p * n)(*[bytes(w) for w in witnesses])
    rb, sb = _blinding_bytes(rs, ss, n)
    out = ctypes.create_string_buffer(256 * n)
    _check(lib().zkr_prove_batch_multi(ks, len(keys), arr, wlen, n, rb, sb, out))
    return [out.raw[256 * i:256 * i + 256] for i in range(n)]


def prove_batch_multi_device(keys, d_witness_ptrs, rs=None, ss=None):
    """zkr_prove_batch_multi_device: the same for witnesses resident in HBM; d_witness_ptrs[i] lives on the device of
    keys[i mod len(keys)] and is complete (synchronise the producer first)."""
    n = len(d_witness_ptrs)
    if n == 0:
        return []
    ks = (ctypes.c_void_p * len(keys))(*[k._h for k in keys])
    arr = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p) for p in d_witness_ptrs])
    rb, sb = _blinding_bytes(rs, ss, n)
    out = ctypes.create_string_buffer(256 * n)
    _check(lib().zkr_prove_batch_multi_device(ks, len(keys), arr, n, rb, sb, out))
    return [out.raw[256 * i:256 * i + 256] for i in range(n)]


def prove_sharded(shards, witness: bytes, r=None, s=None) -> bytes:
    """ONE proof over the shards of a key (ProvingKey.shard(i, parts) at position i), one host thread per shard inside the
    library, partial sums combined on the host (zkr_prove_sharded)."""
    ks = (ctypes.c_void_p * len(shards))(*[k._h for k in shards])
    out = ctypes.create_string_buffer(PROOF_BYTES)
    rb = None if r is None else int(r).to_bytes(32, "little")
    sb = None if s is None else int(s).to_bytes(32, "little")
    _check(lib().zkr_prove_sharded(ks, len(shards), bytes(witness), len(witness), rb, sb, out))
    return out.raw


def prove_sharded_device(shards, d_witness_ptrs, r=None, s=None) -> bytes:
    """The same with the full witness resident on every shard's device (d_witness_ptrs[i] on shards[i].device)."""
    ks = (ctypes.c_void_p * len(shards))(*[k._h for k in shards])
    arr = (ctypes.c_void_p * len(shards))(*[ctypes.c_void_p(p) for p in d_witness_ptrs])
    out = ctypes.create_string_buffer(PROOF_BYTES)
    rb = None if r is None else int(r).to_bytes(32, "little")
    sb = None if s is None else int(s).to_bytes(32, "little")
    _check(lib().zkr_prove_sharded_device(ks, len(shards), arr, rb, sb, out))
    return out.raw


def sharded_split_stats():
    """Of this thread's last sharded proof: None when every shard computed h for itself, else [part][phase] host milliseconds of
    the split calcH's phases (zkr_prove_sharded_split_stats)."""
    parts = ctypes.c_uint(0)
    ms = (ctypes.c_double * 64)()
    _check(lib().zkr_prove_sharded_split_stats(ctypes.byref(parts), ms))
    if parts.value == 0:
        return None
    return [[ms[8 * p + f] for f in range(5)] for p in range(parts.value)]


SHARDED_FORMS = {0: "none", 1: "split", 2: "replicated"}
SHARDED_H_FORMS = {0: "none", 1: "coefficients", 2: "evaluation"}


def sharded_last_form():
    """Which form this thread's last sharded proof took and why (zkr_prove_sharded_last_form): {"form": "split" | "replicated" |
    "none", "reason": one line}.  A sharded proof that fell back to replicated calcH is otherwise only a slower number."""
    form = ctypes.c_int(0)
    buf = ctypes.create_string_buffer(256)
    _check(lib().zkr_prove_sharded_last_form(ctypes.byref(form), buf, 256))
    return {"form": SHARDED_FORMS.get(form.value, str(form.value)), "reason": buf.value.decode()}


def sharded_last_h_form():
    """Which form of H this thread's last sharded proof took and why (zkr_prove_sharded_last_h_form): {"form": "evaluation" |
    "coefficients" | "none", "reason": one line}.  Evaluation form runs when every shard was cut with side_tables=True."""
    form = ctypes.c_int(0)
    buf = ctypes.create_string_buffer(256)
    _check(lib().zkr_prove_sharded_last_h_form(ctypes.byref(form), buf, 256))
    return {"form": SHARDED_H_FORMS.get(form.value, str(form.value)), "reason": buf.value.decode()}


def verify(vk_bin: bytes, proof: bytes, public_signals) -> bool:
    """zkr_verify: the Groth16 pairing check on the host (groth.isValid, common.ts:30-38).  public_signals: ints."""
    pub = b"".join(int(x).to_bytes(32, "little") for x in public_signals)
    ok = ctypes.c_int(0)
    _check(lib().zkr_verify(bytes(vk_bin), len(vk_bin), bytes(proof), pub, len(public_signals), ctypes.byref(ok)))
    return bool(ok.value)


def contribution_check(record: bytes) -> bool:
    """zkr_contribution_check: the record of a delta contribution by itself (host only)."""
    assert len(record) == CONTRIBUTION_BYTES
    ok = ctypes.c_int(0)
    _check(lib().zkr_contribution_check(bytes(record), ctypes.byref(ok)))
    return bool(ok.value)


def _records(records, size) -> bytes:
    rb = bytes(records) if isinstance(records, (bytes, bytearray)) else b"".join(bytes(r) for r in records)
    assert len(rb) % size == 0
    return rb


def contribution_chain_check(records) -> bool:
    """zkr_contribution_chain_check: a chain of delta records (a list of 352-byte records, or their concatenation) from the
    generator on, host only; zkr_hip.lib().zkr_last_error() names the record and the check that failed."""
    rb = _records(records, CONTRIBUTION_BYTES)
    ok = ctypes.c_int(0)
    _check(lib().zkr_contribution_chain_check(rb if rb else None, len(rb) // CONTRIBUTION_BYTES, ctypes.byref(ok)))
    return bool(ok.value)


def vk_contribute(vk_bin: bytes, record: bytes) -> bytes:
    """zkr_vk_contribute: the verifying key that goes with the contributed proving key (vk_delta_2 replaced); raises ZkrError
    for a bad record or one that does not continue this key."""
    assert len(record) == CONTRIBUTION_BYTES
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib().zkr_vk_contribute(bytes(vk_bin), len(vk_bin), bytes(record), ctypes.byref(out), ctypes.byref(n)))
    return _take(out, n.value)


def ptau_new(power: int) -> bytes:
    """zkr_ptau_new: the powers-of-tau transcript of power `power` with tau = alfa = beta = 1 (host only)."""
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib().zkr_ptau_new(power, ctypes.byref(out), ctypes.byref(n)))
    return _take(out, n.value)


def ptau_contribute(ptau: bytes, secrets=None, device=0):
    """zkr_ptau_contribute: -> (the new transcript, the 928-byte record).  secrets: (tau, alfa, beta) as ints with 1 < s < r for
    reproducible tests; None draws them inside the library, where they are wiped before the call returns."""
    sb = None if secrets is None else b"".join(int(x).to_bytes(32, "little") for x in secrets)
    assert sb is None or len(sb) == 96
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    rec = ctypes.create_string_buffer(PTAU_RECORD_BYTES)
    _check(lib().zkr_ptau_contribute(bytes(ptau), len(ptau), sb, device, ctypes.byref(out), ctypes.byref(n), ctypes.cast(rec, ctypes.c_char_p)))
    return _take(out, n.value), rec.raw


def ptau_record_check(records) -> bool:
    """zkr_ptau_record_check: a chain of contribution records (a list of 928-byte records, or their concatenation), host only."""
    rb = bytes(records) if isinstance(records, (bytes, bytearray)) else b"".join(bytes(r) for r in records)
    assert len(rb) % PTAU_RECORD_BYTES == 0
    ok = ctypes.c_int(0)
    _check(lib().zkr_ptau_record_check(rb, len(rb) // PTAU_RECORD_BYTES, ctypes.byref(ok)))
    return bool(ok.value)


def ptau_verify(ptau: bytes, records=(), device=0):
    """zkr_ptau_verify: -> (valid, step, vector); step = the first failed step (0: none), vector = where it was found (0..4:
    tauG1, tauG2, alfaTauG1, betaTauG1, betaG2).  zkr_hip.lib().zkr_last_error() names what failed."""
    rb = bytes(records) if isinstance(records, (bytes, bytearray)) else b"".join(bytes(r) for r in records)
    assert len(rb) % PTAU_RECORD_BYTES == 0
    ok = ctypes.c_int(0)
    rep = (ctypes.c_uint64 * 2)()
    _check(lib().zkr_ptau_verify(bytes(ptau), len(ptau), rb if rb else None, len(rb) // PTAU_RECORD_BYTES, device, ctypes.byref(ok), rep))
    return bool(ok.value), int(rep[0]), int(rep[1])


def points_scale_each(points: bytes, scalars: bytes, g2=False, device=0) -> bytes:
    """zkr_points_scale_each: points[i] <- scalars[i] * points[i] (Montgomery affine points, standard-form scalars below r)."""
    pb = 128 if g2 else 64
    n = len(scalars) // 32
    if len(points) != n * pb or len(scalars) != n * 32:
        raise ValueError("points/scalars length mismatch")
    buf = ctypes.create_string_buffer(bytes(points), len(points))
    _check(lib().zkr_points_scale_each(ctypes.cast(buf, ctypes.c_char_p), bytes(scalars), n, 1 if g2 else 0, device))
    return buf.raw


def points_add_each(points: bytes, addends: bytes, g2=False, device=0) -> bytes:
    """zkr_points_add_each: points[i] <- points[i] + addends[i] (Montgomery affine points; x == 0 is infinity, on either side)."""
    pb = 128 if g2 else 64
    n = len(points) // pb
    if len(points) != n * pb or len(addends) != len(points):
        raise ValueError("points/addends length mismatch")
    buf = ctypes.create_string_buffer(bytes(points), len(points))
    _check(lib().zkr_points_add_each(ctypes.cast(buf, ctypes.c_char_p), bytes(addends), n, 1 if g2 else 0, device))
    return buf.raw


def group_ntt(points: bytes, inverse=False, g2=False, device=0) -> bytes:
    """zkr_group_ntt: the NTT of `ntt` with points for coefficients (Montgomery affine, natural order in and out)."""
    pb = 128 if g2 else 64
    n = len(points) // pb
    logn = n.bit_length() - 1
    if n < 2 or (1 << logn) != n or len(points) != n * pb:
        raise ValueError("length must be a power of two >= 2 points")
    buf = ctypes.create_string_buffer(bytes(points), len(points))
    _check(lib().zkr_group_ntt(ctypes.cast(buf, ctypes.c_char_p), logn, 1 if inverse else 0, 1 if g2 else 0, device))
    return buf.raw


def verify_batch(vk_bin: bytes, proofs, public_signals) -> bool:
    """zkr_verify_batch: True iff every proof verifies under the key (one merged pairing product, host only).
    proofs: list of 256-byte proofs; public_signals: one list of ints per proof."""
    n = len(proofs)
    if n == 0:
        return True
    n_pub = len(public_signals[0])
    assert len(public_signals) == n and all(len(p) == n_pub for p in public_signals)
    pb = b"".join(bytes(p) for p in proofs)
    sb = b"".join(int(v).to_bytes(32, "little") for p in public_signals for v in p)
    ok = ctypes.c_int()
    _check(lib().zkr_verify_batch(bytes(vk_bin), len(vk_bin), pb, sb, n, n_pub, ctypes.byref(ok)))
    return bool(ok.value)


def synth_set_shape(shape: int):
    """0 = rollup-shaped synthetic circuit (default), 1 = dense random (BASELINE configs[4])."""
    _check(lib().zkr_synth_set_shape(shape))


def ntt(data: bytes, inverse=False, device=0) -> bytes:
    n = len(data) // 32
    logn = n.bit_length() - 1
    if n < 2 or (1 << logn) != n:
        raise ValueError("length must be a power of two >= 2 elements")
    buf = ctypes.create_string_buffer(bytes(data), len(data))
    _check(lib().zkr_ntt(buf, logn, 1 if inverse else 0, device))
    return buf.raw


def _msm(fn, pb, points, scalars, device):
    n = len(scalars) // 32
    if len(points) != n * pb:
        raise ValueError("points/scalars length mismatch")
    out = ctypes.create_string_buffer(pb)
    inf = ctypes.c_int()
    _check(fn(bytes(points), bytes(scalars), n, out, ctypes.byref(inf), device))
    return None if inf.value else out.raw


def msm_g1(points: bytes, scalars: bytes, device=0):
    return _msm(lib().zkr_msm_g1, 64, points, scalars, device)


def msm_g2(points: bytes, scalars: bytes, device=0):
    return _msm(lib().zkr_msm_g2, 128, points, scalars, device)


def synth_websnark(log_m, n_public, circuit_seed, toxic_seed, device=0):
    """-> (provingKeyBin, witnessBin) in the binarify.ts layouts (host bytes; small sizes)."""
    p, w = ctypes.c_void_p(), ctypes.c_void_p()
    pl, wl = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib().zkr_synth_websnark(log_m, n_public, circuit_seed, toxic_seed, device, ctypes.byref(p), ctypes.byref(pl),
                                    ctypes.byref(w), ctypes.byref(wl)))
    return _take(p, pl.value), _take(w, wl.value)


def setup_r1cs_websnark(r1cs_bin: bytes, toxic=None, device=0):
    """zkr_setup_r1cs_websnark: Groth16 setup of an R1CS on the GPU, key returned as (provingKeyBin, vk_bin) -- the
    buffer `binarifyProvingKey` would write for the reference's unchanged caller."""
    tb = None if toxic is None else b"".join(int(x).to_bytes(32, "little") for x in toxic)
    pk, vk = ctypes.c_void_p(), ctypes.c_void_p()
    pl, vl = ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib().zkr_setup_r1cs_websnark(bytes(r1cs_bin), len(r1cs_bin), tb, device, ctypes.byref(pk), ctypes.byref(pl), ctypes.byref(vk), ctypes.byref(vl)))
    return _take(pk, pl.value), _take(vk, vl.value)


def synth_witness(log_m, n_public, circuit_seed, witness_seed):
    """Another satisfying witness of the synthetic circuit (host only)."""
    w, wl = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib().zkr_synth_witness(log_m, n_public, circuit_seed, witness_seed, ctypes.byref(w), ctypes.byref(wl)))
    return _take(w, wl.value)


def selftest_f29_forms(field, form, records, device=0):
    """zkr_selftest_f29_forms: records = list of 8-tuples of 9-limb lists (raw 29-bit limbs); returns the 9 result limbs of
    each record as the device computes the product form (0: a b, 1: a^2, 2: a b + c d, 3: a b + c d + e f + g h)."""
    n = len(records)
    flat = (ctypes.c_uint32 * (72 * n))(*[l for rec in records for operand in rec for l in operand])
    out = (ctypes.c_uint32 * (9 * n))()
    _check(lib().zkr_selftest_f29_forms(device, field, form, flat, n, out))
    return [list(out[9 * k:9 * k + 9]) for k in range(n)]


CURVE29_COORDS_IN = (6, 4, 8, 4, 2, 3, 4)  # coordinates of one record per op of zkr_selftest_curve29 (csrc/curve29_raw.hpp)


def curve29_words(g2, op):
    """(words of one record, words of one result) of zkr_selftest_curve29."""
    nl = 18 if g2 else 9
    return CURVE29_COORDS_IN[op] * nl + 2, 3 * nl if op == 5 else 4 * nl + (4 * (16 if g2 else 8) if op == 6 else 0)


def selftest_curve29(g2, op, records, device=0):
    """zkr_selftest_curve29: records = a flat sequence of uint32 words (n records of curve29_words(g2, op)[0] words: raw 29-bit
    limbs of the operation's coordinates, then two flag words); returns (the result words of every record, flat; the n infinity
    flags) as the device computes the group law of csrc/curve29.hpp."""
    rw, ow = curve29_words(g2, op)
    if len(records) % rw:
        raise ValueError("records are not a whole number of %d-word records" % rw)
    n = len(records) // rw
    flat = records if isinstance(records, ctypes.Array) else (ctypes.c_uint32 * len(records))(*records)
    out = (ctypes.c_uint32 * max(1, ow * n))()
    inf = (ctypes.c_uint8 * max(1, n))()
    _check(lib().zkr_selftest_curve29(device, int(bool(g2)), op, flat, n, out, inf))
    return list(out[:ow * n]), list(inf[:n])


FIELD_RAW_OPS_FILE = os.path.normpath(os.path.join(_HERE, "..", "..", "csrc", "field_raw_ops.def"))
FIELD_RAW_RECORD_WORDS = 64   # csrc/field_raw.hpp: 8 operands x 8 words
_field_raw_ops = None


def field_raw_ops():
    """The operations of zkr_selftest_fp as csrc/field_raw_ops.def lists them -- the file the C++ header includes -- as a dict
    name -> (number, operands read, result words)."""
    global _field_raw_ops
    if _field_raw_ops is None:
        import re
        rows = re.findall(r"^ZKR_FIELD_RAW_OP\((\d+),\s*(\w+),\s*(\d+),\s*(\d+)\)", open(FIELD_RAW_OPS_FILE).read(), flags=re.M)
        if not rows or sorted(int(r[0]) for r in rows) != list(range(len(rows))):
            raise ValueError("%s does not number its operations 0 .. n - 1" % FIELD_RAW_OPS_FILE)
        _field_raw_ops = {name: (int(num), int(operands), int(out_words)) for num, name, operands, out_words in rows}
    return _field_raw_ops


def selftest_fp(field, op, records, device=0):
    """zkr_selftest_fp: records = n x 256 bytes (or n x 64 uint32 words as a ctypes array or a sequence): 8 operands of 8 words,
    least significant first; op = a number or a name of field_raw_ops().  Returns the result words of every record as bytes (32 per
    record, 64 for the Fq2 ops) as the device computes csrc/field.hpp on these raw limbs."""
    ops = field_raw_ops()
    num, _, ow = ops[op] if isinstance(op, str) else next((v for v in ops.values() if v[0] == op), (op, 0, 8))
    if isinstance(records, (bytes, bytearray, memoryview)):
        if len(records) % (4 * FIELD_RAW_RECORD_WORDS):
            raise ValueError("records are not a whole number of %d-byte records" % (4 * FIELD_RAW_RECORD_WORDS))
        flat = (ctypes.c_uint32 * max(1, len(records) // 4)).from_buffer_copy(bytes(records) or bytes(4))
        n = len(records) // (4 * FIELD_RAW_RECORD_WORDS)
    else:
        if len(records) % FIELD_RAW_RECORD_WORDS:
            raise ValueError("records are not a whole number of %d-word records" % FIELD_RAW_RECORD_WORDS)
        flat = records if isinstance(records, ctypes.Array) else (ctypes.c_uint32 * max(1, len(records)))(*records)
        n = len(records) // FIELD_RAW_RECORD_WORDS
    out = (ctypes.c_uint32 * max(1, ow * n))()
    _check(lib().zkr_selftest_fp(device, field, num, flat, n, out))
    return bytes(out)[:4 * ow * n]


def _ntt_selftest_desc(desc):
    d = NttSelftestDesc()
    fields = dict(desc)
    fields.setdefault("nbat", 1)
    fields.setdefault("tlog", fields.get("logn", 0) + fields.get("coset_shift", 0))
    for k, v in fields.items():
        if k not in dict(NttSelftestDesc._fields_):
            raise ValueError("zkr_ntt_selftest_desc has no field %r" % k)
        setattr(d, k, int(v))
    return d


def ntt_selftest_words(desc):
    """(words of an input vector, words of an output vector) that zkr_selftest_ntt reads for this descriptor: nbat 2^logn, or for a
    cross pass the 2^klog row blocks end to end -- col_n words each where in_sub / out_sub say the buffers are local.  None for a
    shape whose sizes mean nothing (the C side refuses it before it reads a vector)."""
    d = _ntt_selftest_desc(desc)
    if not (1 <= d.logn <= 22 and d.nbat >= 1 and d.nbat << d.logn <= 1 << 24):
        return None
    if d.cross != 1:
        return d.nbat << d.logn, d.nbat << d.logn
    if not (1 <= d.klog <= 3 and d.klog < d.logn):
        return None
    rows, block = 1 << d.klog, (1 << d.logn) >> d.klog
    return rows * (d.col_n if d.in_sub else block), rows * (d.col_n if d.out_sub else block)


def selftest_ntt(desc, in0, in1=None, out=None, in0_b=None, in1_b=None, out_b=None, device=0):
    """zkr_selftest_ntt: ONE run_ntt (or, with cross=1, ONE run_ntt_cross) of csrc/zkr_prove.hip on these vectors.  desc: a dict of
    the fields of zkr_ntt_selftest_desc (include/zkr.h; tlog defaults to logn + coset_shift, nbat to 1, the rest to 0); the
    vectors: bytes of 32-byte little-endian standard-form words (cross: the row blocks end to end; ntt_selftest_words has the
    lengths), None where the mode takes none.  Every vector is copied to the device and back: returns a dict name -> bytes of what
    each holds after the run -- the raw result in "out" (in place: in "in0"), no bit reversal, no 1/n."""
    d = _ntt_selftest_desc(desc)
    bufs = {}
    for name, v in (("in0", in0), ("in1", in1), ("out", out), ("in0_b", in0_b), ("in1_b", in1_b), ("out_b", out_b)):
        if v is not None:
            v = bytes(v)
            bufs[name] = ctypes.create_string_buffer(v, max(1, len(v)))
    words = ntt_selftest_words(desc)
    if words is not None:   # the lengths the C side will read
        for name, b in bufs.items():
            need = 32 * words[1 if name.startswith("out") else 0]
            if len(b) != need:
                raise ValueError("vector %s has %d bytes, the descriptor asks for %d" % (name, len(b), need))
    arg = lambda name: ctypes.cast(bufs[name], ctypes.c_void_p) if name in bufs else None
    _check(lib().zkr_selftest_ntt(device, ctypes.byref(d), arg("in0"), arg("in1"), arg("out"), arg("in0_b"), arg("in1_b"), arg("out_b")))
    return {name: b.raw for name, b in bufs.items()}


def bench_fq_mul(device=0, legacy=False) -> float:
    """G Fq-mul/s of the hot path's multiplier (9 x 29-bit limbs); legacy=True: the 8 x 32-bit multiplier of field.hpp."""
    v = ctypes.c_double()
    _check((lib().zkr_bench_fq_mul_legacy if legacy else lib().zkr_bench_fq_mul)(device, ctypes.byref(v)))
    return v.value
