/* zkr.h -- C ABI of libzkr_hip.so, the MI355X (gfx950) Groth16 prover behind
 * `wasmBn128.groth16GenProof(witnessBin, provingKeyBin)`.
 *
 * Drop-in boundary (reference call sites, /root/reference = kendricktan/simple-zk-rollups):
 *   operator/src/snarks/common.ts:23   const wasmBn128 = await buildBn128();
 *   operator/src/snarks/common.ts:27   witnessBin   = binarifyWitness(witness)      (binarify.ts:10-48)
 *   operator/src/snarks/common.ts:28   provingKeyBin= binarifyProvingKey(provingKey) (binarify.ts:50-207)
 *   operator/src/snarks/common.ts:29   proof = await wasmBn128.groth16GenProof(witnessBin, provingKeyBin)
 *   scripts/index.js:40,46             second copy of the same call
 * The N-API shim (simple-zk-rollups_amd/napi/zkr_napi.c) binds exactly these entry points; see
 * INTEGRATION.md for the one-line change in common.ts.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  Every function returns 0 on success
 * and a negative zkr_status on failure; zkr_last_error() gives a thread-local message.  All field
 * elements cross the boundary as 32-byte little-endian integers.  "std" = standard form,
 * "mont" = Montgomery form (x * 2^256 mod p), exactly as binarify.ts:78-90 writes key material.
 * There is NO CPU fallback: without a usable HIP device every compute entry point fails with
 * ZKR_ERR_NO_DEVICE.
 */
#ifndef ZKR_H
#define ZKR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  ZKR_OK = 0,
  ZKR_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime error at init */
  ZKR_ERR_BAD_KEY = -2,     /* provingKeyBin header/size/section mismatch (binarify.ts:115-141) */
  ZKR_ERR_BAD_WITNESS = -3, /* witness length != nVars * 32 */
  ZKR_ERR_HIP = -4,         /* HIP runtime failure during a call */
  ZKR_ERR_ARG = -5,         /* null pointer / out-of-range argument */
  ZKR_ERR_DEGENERATE = -6,  /* a proof element is the point at infinity (cannot be serialised) */
  ZKR_ERR_UNSATISFIED = -7  /* circuit inputs violate a constraint (where Circuit.calculateWitness throws) */
} zkr_status;

typedef struct zkr_key zkr_key; /* device-resident proving key (one contiguous HBM arena + workspace) */

/* ---- lifecycle ------------------------------------------------------------------------------ */
const char *zkr_last_error(void);
const char *zkr_version(void);
/* Number of HIP devices visible (0 when none; never fails). */
int zkr_device_count(void);
/* PCI address of HIP device `device` ("0000:c1:00.0"; out_len >= 16): lets a monitoring harness find the device's sysfs
 * node (/sys/bus/pci/devices/<id>: hwmon clock and power) among the GPUs of the node. */
int zkr_device_pci_bus_id(int device, char *out, size_t out_len);

/* Parse a websnark-format proving key (the ArrayBuffer of binarifyProvingKey, binarify.ts:143-206),
 * build the device layout (CSR QAP rows, compacted Montgomery point tables, twiddles) and upload it
 * to `device`.  Replaces the per-call parse inside groth16GenProof (common.ts:28-29). */
int zkr_key_load_websnark(const void *pk_bin, size_t pk_len, int device, zkr_key **out);
void zkr_key_free(zkr_key *key);

/* Key geometry: out[0]=nVars out[1]=nPublic out[2]=domainSize out[3]=nnzA out[4]=nnzB
 * out[5..9]=points kept (non-infinity) in the A,B1,B2,C,H tables. */
int zkr_key_info(const zkr_key *key, uint64_t out[10]);

/* Packed key on disk: the device arena -- CSR rows, window tables, twiddles -- written as is, so a
 * later process loads it with one read + one upload: no JSON, no binarifyProvingKey (binarify.ts:50-207, per call in
 * the reference), no re-parse and no window-table rebuild.  The file is position independent; its header carries
 * a magic and the total length. */
int zkr_key_save(const zkr_key *key, const char *path);
int zkr_key_load_file(const char *path, int device, zkr_key **out);

/* What a device key's arena CONTAINS, not only its header.  level 0: structure (every index a kernel follows stays
 * inside its section); level 1: level 0 + values (points on their curves at every window level, twiddles, canonical
 * coefficients, shared rank maps, header constants).  report (may be null): [0] faulty entries found, [1] section
 * (ZKR_KEYSEC_*), [2] QAP side or table, [3] smallest faulty index.  ZKR_OK, or ZKR_ERR_BAD_KEY with zkr_last_error
 * "key check: <section> <side/table>: <count> bad, first at <index>".
 * Sections, in the order a fault is reported (the first faulty one; structure before values), with what [2] and [3] count:
 *   ROWPTR  CSR row pointers of QAP side [2] (0 = A, 1 = B): row_ptr[0] == 0, non-decreasing, row_ptr[m] == nnz; index = row
 *   COL     column indices of side [2] below nVars; index = term
 *   WIDE    the list of rows wider than the one-thread row kernel takes: strictly increasing, below m, exactly the wide
 *           rows; index = position in the list, or the row for a wide row the list lacks
 *   RANK    rank map of table [2] (0..4 = A, B1, B2, C, H): every entry below the table's point count or "none"; index = scalar
 *   HEADER  a table [2] flagged as identity-ranked whose point count ([3]) differs from its scalar count
 *   POINTS  a stored point of table [2] (any window level) off its curve or not canonical; index = stored point
 *   TWIDDLES [2] = 0: the m-entry table, 1: the local table; an entry differs from the powers of the root; index = entry
 *   COEF    a QAP coefficient of side [2] not below r; index = term
 *   SHARED RANK  the rank map of table [2] is not the identity its header claims, or differs from the map of the table it
 *           shares a digit sort with (B2 with B1, C with A); index = scalar
 *   CONSTS  [2] = 0..4: alfa1, beta1, delta1 (on G1), beta2, delta2 (on the twist and in G2)
 * Level 0 runs by itself on every arena that comes from outside the process: zkr_key_load_file, zkr_key_adopt_arena,
 * zkr_key_adopt_base_arena (and so zkr_key_replicate and zkr_key_shard) refuse an arena that fails it with ZKR_ERR_BAD_KEY. */
enum {
  ZKR_KEYSEC_NONE = 0, ZKR_KEYSEC_ROWPTR = 1, ZKR_KEYSEC_COL = 2, ZKR_KEYSEC_WIDE = 3, ZKR_KEYSEC_RANK = 4, ZKR_KEYSEC_HEADER = 5,
  ZKR_KEYSEC_POINTS = 6, ZKR_KEYSEC_TWIDDLES = 7, ZKR_KEYSEC_COEF = 8, ZKR_KEYSEC_SHARED_RANK = 9, ZKR_KEYSEC_CONSTS = 10
};
int zkr_key_check(const zkr_key *key, int level, uint64_t report[4]);

/* MSM geometry of the device key: window bits c and window count K = ceil(255/c) of the A,B1,B2,C,H tables.  Each
 * table holds K levels per base point (2^(ck) P), so an MSM costs K mixed additions per point. */
int zkr_key_windows(const zkr_key *key, uint32_t c_out[5], uint32_t k_out[5]);

/* Multi-GPU replication: the key is ONE position-independent arena in HBM.
 * rank 0:  zkr_key_arena(key,&ptr,&len)  -> broadcast `len`, then the bytes (RCCL over xGMI)
 * rank k:  zkr_key_adopt_arena(dev_ptr,len,device,&key)  (takes a device pointer holding the bytes;
 *          the caller keeps ownership of that memory and must keep it alive until zkr_key_free). */
int zkr_key_arena(const zkr_key *key, void **dev_ptr, size_t *len);
int zkr_key_adopt_arena(void *dev_ptr, size_t len, int device, zkr_key **out);
/* The same replication with 1/10 of the bytes on the wire: zkr_key_base_arena gives a compact device buffer (owned by
 * the key, valid until zkr_key_free) holding the QAP rows, the BASE points of every table and the rank maps, without
 * the precomputed window levels and twiddles; zkr_key_adopt_base_arena copies it into a full arena on `device` and
 * rebuilds those levels there (about 0.25 s at 2^20).  The caller's buffer may be released as soon as the call returns;
 * the rebuilt arena is byte-identical to the sender's. */
int zkr_key_base_arena(zkr_key *key, void **dev_ptr, size_t *len);
int zkr_key_adopt_base_arena(const void *dev_ptr, size_t len, int device, zkr_key **out);

/* The same replication inside ONE process, device to device (SURVEY.md 8(b) "Threading": one host thread per GPU;
 * 8(e)): the form a Node operator uses -- the reference's host awaits its proofs from one process
 * (operator/src/snarks/common.ts:23-29) -- where no launcher starts a rank per GPU.  Copies `key` (on its own device)
 * to `dst_device` and returns an independent key there (own workspaces; free both with zkr_key_free, in any order).
 * mode FULL: the whole arena in peer copies of at most 1 GiB, adopted as is (nothing recomputed; over xGMI about
 * 30 ms at 2^20); BASE: the compact arena (1/10 of the bytes) and a rebuild of the window levels on dst_device
 * (about 0.1 s at 2^20) -- for device pairs without direct peer access, where the runtime stages the copy through host
 * memory; AUTO: FULL when the devices can address each other (or are the same device), else BASE.  dst_device may be
 * key's own device: a second replica there (two host threads, two proof pipelines on one GPU).  The replica's arena is
 * byte-identical to the source's in every mode. */
enum { ZKR_REPLICATE_AUTO = 0, ZKR_REPLICATE_FULL = 1, ZKR_REPLICATE_BASE = 2 };
int zkr_key_replicate(const zkr_key *key, int dst_device, int mode, zkr_key **out);
/* HIP ordinal of the device the key lives on. */
int zkr_key_device(const zkr_key *key);
/* How the key came to its device: *mode_out = 0 (loaded, built or adopted there) or the form zkr_key_replicate chose
 * (ZKR_REPLICATE_FULL / ZKR_REPLICATE_BASE); *peer_direct_out (may be NULL) = whether source and destination could address each
 * other's memory (0 with FULL: the runtime staged the copy through the host). */
int zkr_key_replication(const zkr_key *key, int *mode_out, int *peer_direct_out);

/* ---- the hot path --------------------------------------------------------------------------- */
/* One Groth16 proof.  witness_std: nVars x 32 B standard form (binarifyWitness layout, host memory).
 * r32/s32: blinding scalars (32 B LE, < r); pass NULL for both to draw them from the OS CSPRNG as
 * the reference does.  proof_out: 256 B = pi_a (x,y) | pi_b (x.re,x.im,y.re,y.im) | pi_c (x,y),
 * affine, standard form -- the eight integers groth16GenProof returns as decimal strings
 * (consumed at common.ts:31-32,44-48).
 * stream: the hipStream_t that produced the witness (e.g. torch.cuda.current_stream().cuda_stream; NULL = the
 * default stream): the proof starts after the work already enqueued there and then runs on the key's own streams. */
int zkr_prove(zkr_key *key, const void *witness_std, size_t witness_len, const uint8_t *r32, const uint8_t *s32,
              uint8_t proof_out[256], void *stream);

/* Same, witness already resident in HBM on the key's device (nVars x 32 B, std form). */
int zkr_prove_device(zkr_key *key, const void *d_witness_std, const uint8_t *r32, const uint8_t *s32,
                     uint8_t proof_out[256], void *stream);

/* Pipelined form for batches of independent proofs (rollup batch, BASELINE config 4): zkr_prove_submit enqueues
 * the whole GPU side of one proof and returns at once with a ticket; zkr_prove_collect waits for that proof and
 * does the host assembly.  A key holds two proof workspaces (zkr_key_slots), so the GPU work of proof i+1 (submitted before
 * collecting proof i) covers proof i's reduction tail and host assembly.  The witness buffer must stay untouched
 * until the ticket is collected.  Submitting with both workspaces in flight fails with ZKR_ERR_ARG.
 * zkr_prove_device(...) == submit + collect. */
int zkr_prove_submit(zkr_key *key, const void *d_witness_std, const uint8_t *r32, const uint8_t *s32, void *stream, int *ticket);
int zkr_prove_collect(zkr_key *key, int ticket, uint8_t proof_out[256]);
/* A whole batch from host buffers (the rollup operator's case: `count` independent witnesses against one key, e.g. the
 * proofs of BASELINE config 4 assigned to this GPU): uploads and proofs pipelined over the key's workspaces.
 * witnesses_std: `count` host pointers to witness_len bytes each; r32s / s32s: count x 32 B blinding scalars or NULL
 * (drawn per proof); proofs_out: count x 256 B.  Stops at the first failing proof (its status is returned). */
int zkr_prove_batch(zkr_key *key, const void *const *witnesses_std, size_t witness_len, size_t count, const uint8_t *r32s, const uint8_t *s32s,
                    uint8_t *proofs_out);
/* The same for witnesses already resident in HBM (count device pointers, nVars x 32 B each; `stream` as for
 * zkr_prove_device).  Both batch calls FUSE proofs of small circuits: a key whose circuit is far below the size that fills
 * the chip (the reference's tx circuit, 2^17 constraints) runs every kernel over up to zkr_key_fuse(key) witnesses at once
 * (vectors end to end, one bucket set per proof and table), so a launch carries about the work of one 2^20 proof and the
 * fixed latency tail of the bucket reduction is paid once per group; two groups are in flight.  Proofs are the same bytes as
 * from zkr_prove_device.  A key with the side tables of the evaluation form (zkr_key_h_form below) runs every group through the
 * four-transform form; a group in which a witness leaves constraints unsatisfied is proved again, whole, through the coefficient
 * form, in its slot and in its proofs' places in the caller's order. */
int zkr_prove_batch_device(zkr_key *key, const void *const *d_witnesses_std, size_t count, const uint8_t *r32s, const uint8_t *s32s, void *stream,
                           uint8_t *proofs_out);
/* A batch over SEVERAL GPUs of the node from one process (BASELINE config 4: 64 independent proofs, 8 per GPU): keys[j] are
 * replicas of one key on n_keys devices (zkr_key_replicate; the same device may appear through two replicas), proof i
 * goes to keys[i mod n_keys], one host thread per key runs zkr_prove_batch / zkr_prove_batch_device on its share (uploads
 * and proofs pipelined per device, small circuits fused), proofs_out keeps the caller's order.  No data moves between
 * the devices.  r32s / s32s as in zkr_prove_batch.  _device: d_witnesses_std[i] is resident on the device of
 * keys[i mod n_keys] and complete when the call is made.  The first failing share's status is returned with its
 * message (prefixed by the key's index and device); the other shares still run to their end. */
int zkr_prove_batch_multi(zkr_key *const *keys, size_t n_keys, const void *const *witnesses_std, size_t witness_len, size_t count, const uint8_t *r32s,
                          const uint8_t *s32s, uint8_t *proofs_out);
int zkr_prove_batch_multi_device(zkr_key *const *keys, size_t n_keys, const void *const *d_witnesses_std, size_t count, const uint8_t *r32s,
                                 const uint8_t *s32s, uint8_t *proofs_out);
/* ---- ONE proof over several GPUs (BASELINE configs[2] and [4] are single proofs) ----------------------
 * The MSMs shard by contiguous ranges: zkr_key_shard cuts every scalar vector of the proof -- the witness w (A, B1, B2, C
 * tables) and the quotient coefficients h (H table) -- into `parts` equal ranges and builds, on `device`, a key holding
 * range `part` of every point table (all window levels; the shard's window size is the one a key of ITS size would choose, so
 * the levels are rebuilt on `device` from the range's base points unless the window stays the same, in which case they are
 * copied device to device) plus the whole QAP and the twiddles: every shard computes h itself ("replicated compute"), so NOTHING is exchanged but the
 * partial sums at the end -- 640 bytes per shard.  The key is sharded, not replicated: a shard holds about 1/parts of the
 * table memory (78 GB at 2^24).
 * zkr_prove_partial(_device) runs a shard's whole share of one proof (host / HBM-resident witness, the FULL witness either
 * way) and returns its partial sums of A, B1, B2 and C + H (ZKR_PARTIAL_BYTES, this library's XYZZ points in Montgomery
 * form: opaque to the caller); zkr_prove_combine adds the `parts` records and does the usual assembly (r32 / s32 as in
 * zkr_prove; `key` = any of the shards, or the whole key: they carry the same alfa, beta, delta).  The proof is the same
 * bytes as zkr_prove's on the whole key.  zkr_prove_sharded(_device): the three steps in one call, one host thread per
 * shard (shards[i] = part i of `parts`; _device: d_witnesses_std[i] = the full witness resident on shard i's device). */
#define ZKR_PARTIAL_BYTES 640
int zkr_key_shard(const zkr_key *key, unsigned part, unsigned parts, int device, zkr_key **out);
/* zkr_key_shard with flags (zkr_key_shard is flags = 0; unknown flags: ZKR_ERR_ARG, before any device call).
 * ZKR_SHARD_SIDE_TABLES: when the whole key has the side tables of the evaluation form (zkr_key_h_form), the shard gets its own on
 * `device`, cut as its point tables are -- E' over its range of the domain (natural order: the range of the whole table), C' over
 * the point range of the table whose digit sort C's accumulation reads, window levels copied when the shard keeps the whole key's
 * window and rebuilt from level 0 otherwise, C by row whole.  zkr_key_h_form then says evaluation for the shard.  The shard is a
 * valid coefficient-form shard all the same (ZKR_OK, zkr_key_h_form says 0, one line in zkr_last_error) when the whole key has no
 * tables, the device has no memory for them, ZKR_H_FORM=coefficients is set, or the shard's C table reads another digit sort than
 * the whole key's.  zkr_key_eval_tables_drop takes a shard; zkr_key_eval_tables does not (derive on the whole key, then cut);
 * zkr_key_eval_tables_equal compares two shards that are the same part of the same cut.
 * Side tables change ONLY zkr_prove_sharded(_device): a shard's partial sums differ between the two forms of H and only their sum
 * over all shards agrees, so zkr_prove_partial(_device) called on its own keeps the coefficient form and its records stay
 * combinable with any shard's.  See zkr_prove_sharded_last_h_form. */
#define ZKR_SHARD_SIDE_TABLES 1u
int zkr_key_shard_opts(const zkr_key *key, unsigned part, unsigned parts, int device, unsigned flags, zkr_key **out);
int zkr_prove_partial(zkr_key *shard, const void *witness_std, size_t witness_len, uint8_t partial_out[ZKR_PARTIAL_BYTES]);
int zkr_prove_partial_device(zkr_key *shard, const void *d_witness_std, void *stream, uint8_t partial_out[ZKR_PARTIAL_BYTES]);
int zkr_prove_combine(zkr_key *key, const uint8_t *partials, size_t parts, const uint8_t *r32, const uint8_t *s32, uint8_t proof_out[256]);
int zkr_prove_sharded(zkr_key *const *shards, size_t parts, const void *witness_std, size_t witness_len, const uint8_t *r32, const uint8_t *s32,
                      uint8_t proof_out[256]);
int zkr_prove_sharded_device(zkr_key *const *shards, size_t parts, const void *const *d_witnesses_std, const uint8_t *r32, const uint8_t *s32,
                             uint8_t proof_out[256]);
/* zkr_prove_sharded(_device) run the shards concurrently, so calcH need not be repeated by every shard: with 2, 4 or 8 shards
 * (each owning one aligned block of h) on devices that can access one another's memory, shard j evaluates 1/parts of the QAP rows
 * and 1/parts of every transform's butterflies; the stages that pair elements of different blocks read and write the other
 * shards' buffers directly (xGMI peer access; shards on one device: plain loads), with a host barrier of the shards' threads
 * between the five phases (four barriers).  The proof is the same bytes.  ZKR_SHARD_SPLIT_H=0: every shard computes h for itself (what
 * zkr_prove_partial on its own always does).  zkr_prove_sharded_split_stats: of the calling thread's last sharded proof --
 * *parts_out = its shards if calcH was split (else 0), phase_ms_out[8 * part + phase] = host time of that shard's phase
 * (enqueue until its stream was idle; phases 0..4 = 1..5 of csrc/zkr_prove.hip calc_h_split, the last one enqueue time only). */
int zkr_prove_sharded_split_stats(unsigned *parts_out, double phase_ms_out[64]);
/* WHICH form the calling thread's last zkr_prove_sharded(_device) took, and why -- a sharded proof that fell back to replicated
 * calcH is otherwise only a slower number: *form_out = ZKR_SHARDED_SPLIT_H / ZKR_SHARDED_REPLICATED_H (NONE: no sharded proof on
 * this thread yet, or it failed before running), reason_out = one line ("no peer access from device 2 to device 5", "3 shards:
 * the split needs 2, 4 or 8", "ZKR_SHARD_SPLIT_H=0", "all shards on one device", ...).
 * Shards on DIFFERENT devices: their first sharded proof runs BOTH forms and compares the sums; the split is kept only if they
 * agree (a warning on stderr and replicated calcH from then on otherwise).  ZKR_SHARD_SPLIT_H=1 skips that check. */
enum { ZKR_SHARDED_NONE = 0, ZKR_SHARDED_SPLIT_H = 1, ZKR_SHARDED_REPLICATED_H = 2 };
int zkr_prove_sharded_last_form(int *form_out, char *reason_out, size_t reason_len);
/* WHICH form of H the calling thread's last zkr_prove_sharded(_device) took (thread-local, as zkr_prove_sharded_last_form;
 * ZKR_H_NONE before any sharded proof on the thread).  Evaluation form -- four transforms instead of six per proof; with a split
 * calcH two cross passes instead of three in phase 2, no cross inverse transform in phase 4, the product on the block in phase 5
 * -- runs iff EVERY shard has side tables (ZKR_SHARD_SIDE_TABLES) and ZKR_H_FORM=coefficients is not set; the first-use check
 * compares split against replicated in the same form.  reason_out, one line: "every shard has side tables", "shard 2 has no side
 * tables", "ZKR_H_FORM=coefficients", or "witness left 3 rows unsatisfied: proved again through the coefficient form" -- the shards
 * count the rows with a_j b_j != c_j (each its block with a split calcH, each all of them otherwise), the counts are summed after the
 * shards' threads have joined, and a witness with such rows is proved again on every shard through the coefficient form: the proof
 * is the same bytes for every witness, and `retries` (zkr_key_h_form) of EVERY shard of the set grows by one. */
enum { ZKR_H_NONE = 0, ZKR_H_COEFFICIENTS = 1, ZKR_H_EVALUATION = 2 };
int zkr_prove_sharded_last_h_form(int *form_out, char *reason_out, size_t reason_len);
/* Measurement only (bench.py's shard leg on a one-GPU box): ONE shard runs its share of a proof with a split calcH ALONE, its own
 * buffers standing in for the other shards' -- the time a shard takes with a GPU to itself and no exchange (*ms_out); what it
 * computes is meaningless and is discarded. */
int zkr_bench_shard_split_solo(zkr_key *shard, const void *d_witness_std, double *ms_out);
/* out[0] = part, out[1] = parts (0, 1 for a whole key), out[2..3] = first scalar and count of the witness range,
 * out[4..5] = the same for h. */
int zkr_key_shard_info(const zkr_key *key, uint32_t out[6]);
/* Number of proof workspaces of the key = submits that can be in flight; proofs one batch submit fuses (1 at 2^20 and above). */
int zkr_key_slots(const zkr_key *key);
int zkr_key_fuse(const zkr_key *key);

/* ---- acceptance check (host only, no GPU) ---------------------------------------------------------
 * The pairing equation `groth.isValid(vk, proof, publicSignals)` evaluates at common.ts:30-38 and
 * TxVerifier.verify evaluates on chain (TxVerifier.sol:258-276):
 *   vk_x = IC_0 + sum_i input_i IC_{i+1};  e(-A, B) e(alfa, beta) e(vk_x, gamma) e(C, delta) == 1.
 * vk_bin: 64 B vk_alfa_1 | 128 B vk_beta_2 | 128 B vk_gamma_2 | 128 B vk_delta_2 | u32 nIC | nIC x 64 B IC, every
 * coordinate a 32-byte LE standard-form integer, G2 as (x.re, x.im, y.re, y.im) (the order of the snarkjs JSON
 * key; index.js / facade.py convert the JSON).  proof: the 256 bytes zkr_prove returns.  public_std: nIC - 1
 * inputs, 32 B each.  *valid = 1 / 0; inputs >= r (TxVerifier.sol:265) and off-curve proof points give 0.
 * Returns an error only for a malformed key or a wrong input count. */
int zkr_verify(const void *vk_bin, size_t vk_len, const uint8_t proof[256], const void *public_std, size_t n_public, int *valid);
/* n_proofs proofs (n_proofs x 256 B) with their public signals (n_proofs x n_public x 32 B) under one key, merged by a
 * random linear combination (128-bit coefficients from the OS CSPRNG) into ONE product of n_proofs + 3 pairings with one
 * final exponentiation: *all_valid = 1 iff every proof verifies (an invalid one slips through with
 * probability 2^-128); about 0.5 ms per proof instead of 3.7.  Use zkr_verify to locate a failing proof, or
 * zkr_verify_each (below) for a verdict per proof. */
int zkr_verify_batch(const void *vk_bin, size_t vk_len, const uint8_t *proofs, const void *publics_std, size_t n_proofs, size_t n_public, int *all_valid);

/* ---- acceptance check on the GPU: a verdict per proof -----------------------------------------------
 * The same equation (common.ts:30-38, TxVerifier.sol:258-276), one proof per lane, where a batch's witnesses already live:
 * zkr_rollup_witness_batch_device -> zkr_r1cs_check_device -> zkr_prove_batch_device -> zkr_verify_each_device.  No random
 * combination: every proof gets its own product of four pairings and its own final exponentiation, so the answer is
 * deterministic and names the proofs that fail.  For every input, verdicts[i] == 0 exactly when zkr_verify on the same key,
 * proof and signals sets *valid = 1.
 *
 * zkr_vk_load: vk_bin in the layout of zkr_verify, read by the same parser with the same bounds and messages, BEFORE any device
 * call: a malformed key is ZKR_ERR_BAD_KEY (ZKR_ERR_ARG for a key without an IC point) on a machine without a GPU too, a
 * well-formed one without a device ZKR_ERR_NO_DEVICE (no CPU fallback).  nPublic is the key's IC count less one.  The handle
 * owns, on `device`: the 8-bit window table of the IC points (255 affine multiples each), the prepared lines of beta, gamma
 * and delta, the Miller value of (alfa, beta), the constants of the pairing, one stream, and per-batch buffers that grow to
 * the largest batch seen (about 4 KiB + nPublic x 32 B per proof).  One zkr_vk serves ONE call at a time, as a zkr_r1cs does;
 * two handles (of the same key too) run concurrently.
 * zkr_vk_info: out[0] = nPublic, out[1] = device. */
typedef struct zkr_vk zkr_vk;
int zkr_vk_load(const void *vk_bin, size_t vk_len, int device, zkr_vk **out);
void zkr_vk_free(zkr_vk *vk);
int zkr_vk_info(const zkr_vk *vk, uint64_t out[2]);
/* The first check that fails, in the order zkr_verify makes them:
 *   BAD_G1     A or C: a coordinate not below q, the point at infinity, off the curve;
 *   BAD_INPUT  a public signal not below r (TxVerifier.sol:265);
 *   BAD_G2     B: a coordinate not below q, infinity, off the twist, or outside the order-r subgroup;
 *   EQUATION   e(-A, B) e(alfa, beta) e(vk_x, gamma) e(C, delta) != 1. */
enum { ZKR_VERDICT_VALID = 0, ZKR_VERDICT_BAD_G1 = 1, ZKR_VERDICT_BAD_INPUT = 2, ZKR_VERDICT_BAD_G2 = 3, ZKR_VERDICT_EQUATION = 4 };
#define ZKR_VERIFY_PIECE 4096 /* proofs per set of launches: a larger batch is cut into pieces of this size inside the call */
/* proofs: n_proofs x 256 B in HOST memory (where zkr_prove_batch* leave them).  publics_std: n_proofs x nPublic x 32 B in host
 * memory (may be NULL when nPublic == 0).  verdicts: n_proofs bytes, may be NULL.  *all_valid = 1 iff every verdict is 0;
 * n_proofs == 0 is ZKR_OK with *all_valid = 1.  An invalid proof is NOT an error status: ZKR_OK, and zkr_last_error names the
 * first one ("proof 17: pairing equation fails", "proof 3: B is not in the order-r subgroup").  A status below zero only for
 * null pointers (ZKR_ERR_ARG) or a HIP failure. */
int zkr_verify_each(zkr_vk *vk, const uint8_t *proofs, const void *publics_std, size_t n_proofs, uint8_t *verdicts, int *all_valid);
/* The same with the public signals read in place: d_witnesses_std holds n_proofs device pointers on the key's device (a host
 * array), proof i's signals are words 1..nPublic of witness i.  Nothing comes back to the host but the verdicts.  A witness word
 * is judged as it stands and NOT reduced: a word >= r is BAD_INPUT, which is what the contract answers (zkr_r1cs_check_device
 * reduces it first and may accept the same witness).  stream: as for zkr_prove_device and zkr_r1cs_check_device -- the check
 * starts after the work already queued there and runs on the handle's own stream; the call returns when the verdicts are on the
 * host.  A null witness pointer is ZKR_ERR_ARG. */
int zkr_verify_each_device(zkr_vk *vk, const uint8_t *proofs, const void *const *d_witnesses_std, size_t n_proofs, void *stream,
                           uint8_t *verdicts, int *all_valid);

/* ---- stage hooks (tests, profiling) ----------------------------------------------------------- */
/* e(P_i, Q_i) after the final exponentiation, one pair per lane (the arithmetic of zkr_verify_each by itself).  g1_std: n x 64 B,
 * g2_std: n x 128 B (x.re, x.im, y.re, y.im), standard-form affine; an all-zero point is infinity and gives one.  The points are
 * taken as given: the caller vouches for curve and subgroup.  out: n x 384 B, the twelve Fq coefficients in standard form in the
 * tower's order Fq12 = c0 + c1 w, Fq6 = c0 + c1 v + c2 v^2, Fq2 = a + b u:
 *   c0.c0.a, c0.c0.b, c0.c1.a, c0.c1.b, c0.c2.a, c0.c2.b, c1.c0.a, ..., c1.c2.b    (w^2 = v, v^3 = 9 + u, u^2 = -1).
 * degenerate[i] (may be NULL) = 1 when the projective Miller loop of pair i met Z = 0 (impossible for a Q of order r). */
int zkr_pairing_device(const void *g1_std, const void *g2_std, size_t n, void *out, uint8_t *degenerate, int device);
/* In-place NTT of n = 2^logn standard-form elements in host memory; natural order in and out (words >= r are reduced first). */
int zkr_ntt(void *data_std, unsigned logn, int inverse, int device);
/* sum_i scalars[i] * points[i].  points: Montgomery affine as in the key sections (64 B G1 / 128 B G2;
 * x == 0 encodes infinity, binarify.ts:92-102); scalars: std 32 B.  out: std affine; *is_inf set when
 * the sum is the point at infinity. */
int zkr_msm_g1(const void *points_mont, const void *scalars_std, size_t n, uint8_t out[64], int *is_inf, int device);
int zkr_msm_g2(const void *points_mont, const void *scalars_std, size_t n, uint8_t out[128], int *is_inf, int device);
/* h = upper-half coefficients of A(x)B(x), natural order, std form, m x 32 B. */
int zkr_calc_h(zkr_key *key, const void *witness_std, size_t witness_len, void *h_out);

/* Per-stage device timing, measured with hipEvents on the launch stream.  Stage names:
 * "ingest","spmv","ntt","msm_sort","msm_accum_g1","msm_accum_g2","msm_big","msm_reduce","total".
 * "msm_accum_g1"/"msm_accum_g2" bracket exactly one msm_accum_kernel launch each time. */
int zkr_prof_enable(zkr_key *key, int on);
int zkr_prof_reset(zkr_key *key);
int zkr_prof_get(zkr_key *key, const char *stage, double *ms_total, uint64_t *launches);

/* ---- synthetic workload + device-side setup (benchmarks) -------------- */
/* Rollup-shaped seeded R1CS + witness + Groth16 key generated from seeded toxic waste, key points
 * computed ON DEVICE by fixed-base multiplication (the websnark binary is never materialised, so
 * this works past its 4 GiB u32-offset limit).  witness_out: malloc'ed nVars x 32 B std (free with
 * zkr_free).  aux_out (optional, may be NULL): malloc'ed blob for the checker --
 *   u64 nVars | 5 x 32 B toxic (t,alfa,beta,gamma,delta) | nVars x 32 B a_s | b_s | c_s  (std form)
 *   | (nPublic+1) x 64 B IC points (std affine) | 128 B vk_gamma_2 (std) */
int zkr_synth_key(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t toxic_seed, int device,
                  zkr_key **key_out, void **witness_out, size_t *witness_len, void **aux_out, size_t *aux_len);
/* Verifying key of a zkr_synth_key key in the vk_bin layout of zkr_verify (malloc'ed, free with zkr_free);
 * aux = the checker blob zkr_synth_key returned for this key. */
int zkr_synth_vk(const zkr_key *key, const void *aux, size_t aux_len, void **vk_out, size_t *vk_len);
/* Same circuit + setup rendered as a websnark-format key on the host (small sizes; tests). */
int zkr_synth_websnark(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t toxic_seed, int device,
                       void **pk_out, size_t *pk_len, void **witness_out, size_t *witness_len);
/* Another satisfying witness of the same synthetic circuit (host only, no GPU): structure comes from
 * circuit_seed, free values from witness_seed (zkr_synth_key uses witness_seed = circuit_seed). */
int zkr_synth_witness(unsigned log_m, unsigned n_public, uint64_t circuit_seed, uint64_t witness_seed, void **witness_out,
                      size_t *witness_len);
/* Groth16 trusted setup of an arbitrary R1CS, key elements computed on the GPU: what
 * `snarkjs setup --protocol groth -c build/tx.json --pk ... --vk ...` does in the reference's workflow
 * (prover/package.json:34,37), producing the device key directly (no JSON, no binarifyProvingKey) and the verifying key
 * in the vk_bin layout of zkr_verify.  r1cs_bin: u32 nVars | u32 nPublic (outputs + public inputs) | u32 nConstraints |
 * per constraint, for each of A, B, C: u32 k, then k x (u32 signal, 32 B coefficient, standard form LE) -- the
 * `constraints` array of circom's circuit JSON (index.js / facade.py convert it).  toxic160: t, alfa, beta, gamma,
 * delta (5 x 32 B, non-zero, < r) for reproducible test setups, or NULL to draw them from the OS CSPRNG inside the call
 * (they are wiped before it returns).  domainSize = smallest power of two >= nConstraints + nPublic + 1. */
int zkr_setup_r1cs(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, zkr_key **key_out, void **vk_out, size_t *vk_len);
/* H in evaluation form.  A builder that knows the key's scalars (zkr_setup_r1cs with toxic scalars or its own, zkr_synth_key) also
 * builds two side tables beside the arena, with the window plans of C and H: C' = C + 1/2 C^T F over all nVars signals and
 * E' = -1/2 E over the domain, the H table moved to the evaluations on the coset by two transforms of its scalars.  A whole-key proof
 * -- of its own launches, or in a fused group of the batch calls -- then runs four transforms instead of six: the H multiexp takes the coset products A(g w^j) B(g w^j) as they
 * are, the C multiexp takes the witness over C'.  That rests on a o b = C w, so every such proof also counts the rows where it
 * fails (one count per proof of a fused group), and a witness with such rows is proved again through the coefficient form, in its
 * place in the caller's order -- with the rest of its group, when it came in one: the proof is the same bytes for every witness.
 * A shard proving on its own (zkr_prove_partial) and the stage hooks (zkr_calc_h) keep the coefficient form; a sharded proof takes the
 * evaluation form when every shard was cut with side tables (zkr_key_shard_opts).  The tables cost about as much device memory as C and H themselves (2 x 0.87 GB at 2^20);
 * when they cannot be allocated, or a signal of C' has no point in the layout C shares, the key simply keeps the coefficient
 * form (ZKR_H_FORM=coefficients asks for that).  They are not part of the arena: key files, replicas, shards, contributed keys
 * (zkr_key_contribute changes C and H), websnark-loaded and transcript keys come without them and prove through the coefficient
 * form until zkr_key_eval_tables (below) derives the tables from the key's own points.
 * zkr_key_h_form: *evaluation = 1 when the key has the tables; *retries = witnesses of this key that left rows unsatisfied and were
 * proved again so far -- the witnesses that failed, not the proofs of their groups that went again with them, so the count does not
 * depend on how a batch was cut into groups (either may be NULL).
 * zkr_setup_r1cs_opts: zkr_setup_r1cs with flags; ZKR_SETUP_NO_SIDE_TABLES refuses the side tables' allocation (a test hook for
 * the fall-back). */
#define ZKR_SETUP_NO_SIDE_TABLES 1u
int zkr_setup_r1cs_opts(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, unsigned flags, zkr_key **key_out, void **vk_out, size_t *vk_len);
int zkr_key_h_form(const zkr_key *key, int *evaluation, uint64_t *retries);
/* The same side tables for ANY whole key -- loaded from websnark bytes or a file, made from a transcript, replicated, contributed to --
 * from the key's own points and the circuit's C side; no scalar of the setup is needed.  Both tables are linear images of points the
 * key holds: E'_j = ke 1/m sum_i (g w^j)^(-i) H_i (ke = -1/2 R / m^2) is the H points scaled one by one and taken through one inverse
 * NTT over points; C'_s = C_s + 1/2 sum_j C_js F_j, F_j = 1/m sum_i w^(-ij) H_i, is a second such transform, one sparse combination
 * over the columns of C and one addition per signal.  All on the key's device, once per key (the cost is that of two G1 transforms
 * over the domain).  The tables are the bytes of the ones zkr_setup_r1cs builds for the same key.
 * r1cs_bin: the layout of zkr_setup_r1cs; it is parsed before any device call.  ZKR_ERR_ARG: a null pointer, flags other than 0, a
 * malformed system, a shard key, a system whose nVars, nPublic or domain differ from the key's, a key with a proof in flight (a slot
 * submitted and not collected).  *built = 1: the key has the tables, and zkr_key_h_form reports evaluation from then on.
 * ZKR_OK with *built = 0 and a one-line reason in zkr_last_error where the setup's builder gives up as well: ZKR_H_FORM=coefficients,
 * an H table that dropped a point, a signal with a finite C' point and no slot among the points C's accumulation reads, no memory
 * for the tables.  A status below zero otherwise only for a failed kernel or copy.  A key that has tables drops them first.
 * WHICH C matrix: the identity the tables rest on holds for any matrix M with M w = a o b, and every evaluation-form proof checks
 * exactly that of its witness.  A wrong or stale C side therefore gives no wrong proof: it makes every proof take the retry path
 * (slower; `retries` of zkr_key_h_form counts them), alone or as fused groups.  Nothing binds r1cs_bin to the key beyond its geometry.
 * Loading, saving, replicating and contributing carry no tables, as before: derive again on the key such a step returns; a shard
 * gets its part of them only through zkr_key_shard_opts with ZKR_SHARD_SIDE_TABLES.
 * zkr_key_eval_tables_drop: back to the coefficient form; frees the tables (ZKR_ERR_ARG with a proof in flight).
 * zkr_key_eval_tables_equal (test hook): *same = 1 iff both keys, on one device, have tables and their C' and E' tables at every window
 * level and their C rows are equal byte for byte.
 * zkr_points_add_each (stage hook, as zkr_points_scale_each below): points[i] <- points[i] + addends[i], n points in host memory,
 * Montgomery affine (64 B G1 / 128 B G2; x == 0 encodes infinity, which either side, or both, may be; equal and opposite points are
 * handled); an infinite sum is written as all zeros. */
int zkr_key_eval_tables(zkr_key *key, const void *r1cs_bin, size_t r1cs_len, unsigned flags, int *built);
int zkr_key_eval_tables_drop(zkr_key *key);
int zkr_key_eval_tables_equal(const zkr_key *a, const zkr_key *b, int *same);
int zkr_points_add_each(void *points_mont, const void *addends_mont, size_t n, int g2, int device);
/* The same setup, delivering the proving key as the bytes `binarifyProvingKey(provingKey)` produces from snarkjs' JSON key
 * (binarify.ts:143-206; malloc'ed, free with zkr_free; at most 4 GiB, the format's u32 offsets) instead of a device key:
 * the provingKeyBin an UNCHANGED reference caller passes to groth16GenProof on every call (common.ts:28-29). */
int zkr_setup_r1cs_websnark(const void *r1cs_bin, size_t r1cs_len, const uint8_t *toxic160, int device, void **pk_out, size_t *pk_len, void **vk_out,
                            size_t *vk_len);

/* ---- a device key back in the reference's format (the way out that zkr_key_load_websnark is the way in of) ---------
 * zkr_key_export_websnark: the same bytes (binarify.ts:143-206; malloc'ed, free with zkr_free) for ANY whole key -- loaded from
 * websnark bytes or a key file, adopted, replicated in either mode, set up from scalars or from a transcript, contributed -- so a
 * key no party can forge for (zkr_setup_r1cs_ptau + zkr_key_contribute) reaches groth16GenProof and the checkers.  n, p, m and the
 * 448 constant bytes come from the arena header; polsA / polsB from the CSR sides: per signal by constraint index ascending, terms
 * of one (signal, row) in their stored order, zero coefficients and duplicates as stored, the input-consistency rows like any
 * other; the five point sections from level 0 of the window tables through the rank maps, on the GPU.  A scalar without a point
 * (dropped at load, or the placeholder of a table laid out over a shared support) is the point at infinity as binarify.ts:92-102
 * writes snarkjs's [0, 1, 0]: x = 0, y = Montgomery one; G2: x = (0, 0), y = (one, 0).  The side tables of the evaluation form
 * are not part of the format.  ZKR_EXPORT_STANDARD: every field element in standard form instead of Montgomery -- not websnark
 * bytes but the raw material of snarkjs's JSON key; infinity is (0, 1) and ((0, 0), (1, 0)).
 * piece_points: output points per table converted and copied at a time (0: 2^20).  The call owns one device staging buffer of
 * that many G2 points, one pinned buffer and one stream, and leaves nothing allocated; it only reads the arena, so proofs of the
 * key may be in flight.  ZKR_ERR_ARG with a message: a null pointer, an unknown flag (both before any device call), a shard ("a
 * shard holds a range of the tables"), a key past the format's 4 GiB (decided from the header before anything is allocated).
 * zkr_key_export_last_times: this thread's last export -- [0] kernels, [1] copies, [2] host writer, [3] total, milliseconds,
 * [4] the extra device bytes it held.
 * Host only, the format's arithmetic and writer on their own: zkr_websnark_len is the length of a key with these sizes (nnz: the
 * terms of a side, input-consistency rows included), ZKR_ERR_ARG past 2^32 - 1; zkr_websnark_render_host writes the bytes from the
 * two sides in CSR by row (rowptr: domain + 1 entries from 0 to the side's term count; col: the signal; coef: 32 B, copied as they
 * are) and the five full-length point sections in wire order A, B1, B2, C, hExps (n, n, n, n - p - 1, m points). */
#define ZKR_EXPORT_STANDARD 1u
typedef struct {
  uint32_t flags;
  uint32_t piece_points;
} zkr_key_export_opts; /* NULL or zeros: defaults */
int zkr_key_export_websnark(const zkr_key *key, const zkr_key_export_opts *opts, void **pk_out, size_t *pk_len);
int zkr_key_export_last_times(double out[5]);
int zkr_websnark_len(uint64_t n_vars, uint64_t n_public, uint64_t domain, uint64_t nnz_a, uint64_t nnz_b, uint64_t *len);
int zkr_websnark_render_host(uint32_t n_vars, uint32_t n_public, uint32_t domain, const uint8_t *consts448, const uint32_t *rowptr_a, const uint32_t *col_a,
                             const uint8_t *coef_a, const uint32_t *rowptr_b, const uint32_t *col_b, const uint8_t *coef_b, const uint8_t *const points[5],
                             void **pk_out, size_t *pk_len);

/* ---- does a witness satisfy its constraint system? (`snarkjs wtns check`, on the GPU) ----------------------------
 * zkr_prove proves whatever witness it is given: the key holds the A and B sides of the QAP and no C side, the quotient divides
 * exactly for every witness, and a witness that violates the circuit gives ZKR_OK and 256 bytes no verifier accepts.  The
 * reference stands two things beside its prover: `Circuit.calculateWitness` (operator/src/snarks/common.ts:15-17), which throws
 * on inputs that violate the circuit it was compiled from, and `groth.isValid` after every proof (common.ts:30-38), which answers
 * "invalid" and never where.  The witness builders of this library (zkr_rollup_witness*) stand in for the first for this build's
 * own two circuits only; zkr_r1cs_check stands in for it for ANY system and witness producer, before the proof, on the device
 * where batch witnesses already live (zkr_rollup_witness_batch_device -> zkr_r1cs_check_device -> zkr_prove_batch_device), and
 * names the first violated constraint.
 * zkr_r1cs_load: r1cs_bin in the layout of zkr_setup_r1cs, parsed by the same parser (same bounds, same messages) BEFORE any
 * device call -- a malformed buffer is ZKR_ERR_ARG on a machine without a GPU too, a well-formed one without a device
 * ZKR_ERR_NO_DEVICE (no CPU fallback).  The system stays on `device`: three CSR sides with Montgomery coefficients, the list of
 * wide constraints, a small result buffer.  Nothing is normalised: a signal that appears twice in one side adds up, an empty
 * side is zero.  zkr_r1cs_info: out[0..5] = nVars, nPublic, nConstraints, terms of A, of B, of C.
 * One zkr_r1cs serves ONE call at a time (it owns one stream and one result buffer, as a key owns its proof workspaces): calls on
 * the same system from several host threads must be serialised by the caller; different systems are independent. */
typedef struct zkr_r1cs zkr_r1cs;
int zkr_r1cs_load(const void *r1cs_bin, size_t r1cs_len, int device, zkr_r1cs **out);
void zkr_r1cs_free(zkr_r1cs *cs);
int zkr_r1cs_info(const zkr_r1cs *cs, uint64_t out[6]);
/* The check.  Witnesses: nVars x 32 B standard form, exactly what zkr_prove(_device) takes; _device: `count` pointers into HBM
 * on the system's device, `stream` as for zkr_prove_device (the check starts after the work already queued there -- the witness
 * producer -- and runs on the system's own stream); the call returns once the reports are on the host.  The host form uploads the
 * witnesses (witness_len != nVars * 32: ZKR_ERR_BAD_WITNESS) and calls the device form.
 * reports (may be NULL): count x 3 words per witness:
 *   [0] constraints violated   [1] the smallest violated constraint (UINT64_MAX: none)   [2] 1 when signal 0 is not 1
 * *all_satisfied = 1 iff every witness has [0] == 0 and [2] == 0.
 * What is judged is the witness the prover would use: every word is reduced below r first (a word w + r gets the verdict of w).
 * Signal 0 must be 1: the verifier's IC_0 assumes it, and a consistent witness with w[0] = 2 satisfies every constraint and still
 * proves nothing.  A violated witness is NOT an error status (as with zkr_verify): ZKR_OK, *all_satisfied = 0 and a
 * zkr_last_error line for the first failing witness, "witness 2: 3 constraints violated, first 492" or "witness 0: signal 0 is
 * not 1".  A status below zero only for bad arguments (count == 0 and null pointers: ZKR_ERR_ARG) or a HIP failure. */
int zkr_r1cs_check_device(zkr_r1cs *cs, const void *const *d_witnesses_std, size_t count, void *stream, uint64_t *reports, int *all_satisfied);
int zkr_r1cs_check(zkr_r1cs *cs, const void *const *witnesses_std, size_t witness_len, size_t count, uint64_t *reports, int *all_satisfied);
/* Which key a system belongs to -- nothing else stops a caller from checking witnesses against the wrong or a stale circuit file.
 * *same = 1 iff nVars and nPublic agree, the key's domain is the one zkr_setup_r1cs's rule gives the system, and for ONE random
 * vector v of nVars field elements (OS CSPRNG) the key's QAP sides, evaluated by the prover's own row kernels over the key's
 * arena, agree word for word with the system: A v on the rows below nConstraints, v[s] on row nConstraints + s for s <= nPublic
 * (the rows snarkjs's setup appends), zero above; B v on the rows below nConstraints, zero above.  Two different matrices agree
 * on a random v with probability 1/r; term order inside a row does not matter.
 * WHAT THIS BINDS: the A and B sides only.  A key has no C side to compare -- C reaches a key only through the C-query points of
 * its setup -- so a system that differs from the key's in C alone is reported as the same.  The call catches the wrong or stale
 * circuit file; it is no statement about the key's C query (zkr_key_audit makes that one, against the transcript the key came from).
 * A shard key is accepted (it holds the whole QAP).  Key and system on different devices: ZKR_ERR_ARG.  A mismatch is ZKR_OK with
 * *same = 0 and a zkr_last_error line naming the geometry, or the side and the first differing row. */
int zkr_r1cs_matches_key(zkr_r1cs *cs, const zkr_key *key, int *same);

/* ---- witness programs: batch witnesses for ANY circuit on the GPU (csrc/zkr_wprog.hip over csrc/wprog.hpp) ----
 * zkr_setup_r1cs, zkr_r1cs_check, zkr_prove* and zkr_verify_each take any circuit; the witness builders of this library
 * (zkr_rollup_witness*, zkr_withdraw_witness*) are device programs written by hand for its own two.  A witness program is the
 * same thing as DATA: r1cs_bin carries a circuit's constraints, wprog_bin carries how its values are computed, and a front end
 * emits the two from one description (python/zkr_hip/circuit.py is one; a converter from circom's output would be another).
 *
 * wprog_bin.  All integers little-endian u32.  The program is straight-line -- no control flow -- over a store of WIRES, which
 * are Fr values numbered implicitly: wire 0 is the constant 1, wires 1..n_inputs are the instance's inputs in order, and every
 * value-producing instruction defines the next wire.  Every wire an instruction names must be an EARLIER wire.
 *   header   u32 magic 0x50574b5a ("ZKWP") | u32 version = 1 | u32 n_inputs | u32 n_consts | u32 n_instr |
 *            u32 n_vars | u32 n_public | u32 n_statements
 *   consts   n_consts x 32 B, standard form LE, below r
 *   code     n_instr x 16 B:  u32 op | u32 a | u32 b | u32 c     (a field an opcode does not use is 0)
 *   map      n_vars x u32: witness signal s of an instance is the value of wire map[s]; map[0] = 0
 * and nothing after it.  Opcodes:
 *   1 CONST k        the value of constant-pool entry a = k
 *   2 ADD a b   3 SUB a b   4 MUL a b     field arithmetic on wires a and b
 *   5 INV0 a         0 for 0, the inverse otherwise
 *   6 BIT a i        bit b = i < 254 of the canonical standard-form value of wire a, as 0 or 1
 *   7 ASSERT_ZERO a stmt     defines no wire: the first such instruction in program order whose wire a is not zero sets the
 *                    instance's statement to b = stmt < n_statements
 * Division is MUL with INV0; comparators, selectors and hashes are compositions: the front end's business.  n_public and
 * n_statements are carried for the caller (the circuit's nPublic; how many statement texts the front end keeps).
 * THE VALIDATOR runs before any device call, so a malformed program is ZKR_ERR_ARG with a message naming the field on a machine
 * without a GPU too: magic, version, the exact length the counts give; every count at most 2^28 and 1 + n_inputs + n_instr at
 * most 2^28; n_public < n_vars; every constant below r; per instruction a known opcode, every wire operand below the wire the
 * instruction would define, a constant index below n_consts, a bit index below 254, a statement below n_statements, unused
 * fields 0; every map entry below the wire count, entry 0 = wire 0.  The kernels index device memory with the program's numbers
 * and check none of them: this validation is why they cannot read or write out of bounds.
 *
 * zkr_wprog_load: parse and validate, then the device (ZKR_ERR_NO_DEVICE without one: no CPU fallback); uploads the code, the
 * constants in Montgomery form and the map, and allocates the handle's one workspace: the wire store, n_wires x piece x 32 B, and
 * piece x 8 B of reports.  A batch is processed in pieces of `piece` instances.  zkr_wprog_load_opts: opts->piece = 0 (and
 * zkr_wprog_load) takes the DEFAULT: the largest multiple of 64 whose store fits 1 GiB, at least 64 and at most 16384; any
 * other value up to 2^20 is taken as it is (a store that cannot be allocated is ZKR_ERR_HIP).  reserved must be 0.
 * One zkr_wprog serves ONE call at a time (it owns one stream and one workspace, as a zkr_r1cs does).
 * zkr_wprog_info: out[0..7] = n_inputs, wires, instructions, n_vars, n_public, workspace bytes held, piece, n_statements.
 * zkr_wprog_shape: the same from the bytes alone, host only (out[5] = out[6] = 0).
 * zkr_wprog_witness_batch_device: d_inputs_std = n x n_inputs x 32 B, standard form, in device memory; d_witnesses = device
 * memory for n x n_vars x 32 B, standard form -- exactly what zkr_prove_batch_device, zkr_r1cs_check_device and
 * zkr_verify_each_device take.  Both 16-byte aligned.  `stream` as for zkr_prove_device: the work starts after what is queued
 * there (the producer of the inputs) and runs on the handle's own stream; the call returns when the witnesses are complete.
 * reports (may be NULL): n x 2 words: [0] 0 ok, 1 an input is not below r ([1] = the first such input), 2 an assertion failed
 * ([1] = its statement).  When an instance fails the status is ZKR_ERR_UNSATISFIED and zkr_last_error names the FIRST failing
 * instance, "instance 64 violates statement 3" or "instance 0: input 2 is not below r"; the witnesses of the instances that did
 * not fail are complete and correct all the same, those of the failing ones are all zero.  n = 0 is ZKR_OK, nothing launched.
 * zkr_wprog_witness_batch: the same with the inputs in host memory; their range check then happens on the host before the device
 * is looked at: ZKR_ERR_ARG naming the first element not below r, nothing launched (as zkr_babyjub_pubkey_batch).
 * zkr_wprog_stage_times: milliseconds the last batch call spent in the interpreter kernel and in the layout kernel (events on the
 * handle's stream, summed over the pieces).
 * zkr_wprog_run_host: test hook -- ONE instance on the host through the same interpreter step, no device.  witness_out: n_vars x
 * 32 B (all zero unless *code = 0); wires_out (may be NULL): every wire, standard form (all zero for code 1).  ZKR_OK whatever
 * the instance's *code; ZKR_ERR_ARG for a malformed program.
 * zkr_mimcsponge_round_constants: the 220 round constants of zkr_mimcsponge_multihash (220 x 32 B, standard form), for front ends
 * that compose the hash.  The Node binding does not carry these calls. */
typedef struct zkr_wprog zkr_wprog;
typedef struct zkr_wprog_opts {
  uint32_t piece;     /* instances per pass over the wire store; 0: the default */
  uint32_t reserved;  /* 0 */
} zkr_wprog_opts;
int zkr_wprog_load(const void *wprog_bin, size_t len, int device, zkr_wprog **out);
int zkr_wprog_load_opts(const void *wprog_bin, size_t len, int device, const zkr_wprog_opts *opts, zkr_wprog **out);
void zkr_wprog_free(zkr_wprog *prog);
int zkr_wprog_info(const zkr_wprog *prog, uint64_t out[8]);
int zkr_wprog_shape(const void *wprog_bin, size_t len, uint64_t out[8]);
int zkr_wprog_witness_batch_device(zkr_wprog *prog, const void *d_inputs_std, size_t n, void *d_witnesses, uint32_t *reports, void *stream);
int zkr_wprog_witness_batch(zkr_wprog *prog, const uint8_t *inputs_std, size_t n, void *d_witnesses, uint32_t *reports);
int zkr_wprog_stage_times(const zkr_wprog *prog, double out_ms[2]);
int zkr_wprog_run_host(const void *wprog_bin, size_t len, const uint8_t *inputs_std, uint8_t *witness_out, uint8_t *wires_out, uint32_t *code, uint32_t *stmt);
int zkr_mimcsponge_round_constants(uint8_t *out);

/* ---- a further party's contribution to a key's delta (what makes a key somebody else can trust) ------
 * Whoever ran a setup saw (or chose) delta, and delta forges proofs (a key from a transcript has delta = 1).  A contributor
 * re-randomises delta with a secret d of its own and none of the toxic values:
 *   delta1' = d delta1, delta2' = d delta2, C'[s] = d^-1 C[s] (s > nPublic), hExps'[i] = d^-1 hExps[i]; vk_delta_2' = d vk_delta_2
 * -- exactly the key a setup with delta d would have produced (byte for byte).  It protects against the earlier holders of
 * DELTA only: a key from zkr_setup_r1cs stays forgeable by whoever knows t, alfa and beta (hExps[0] = Z(t)/delta G1 hands the
 * runner of the setup (1/delta') G1 whatever d was).  A key from zkr_setup_r1cs_ptau followed by at least one zkr_key_contribute
 * is sound if ONE phase-1 contributor of the transcript and ONE delta contributor forgot their secrets.
 * The record (ZKR_CONTRIBUTION_BYTES; every coordinate 32 B LE standard form, as in vk_bin):
 *   delta1_before (64) | delta1_after (64) | delta2_after (128) | R (64) | z (32)
 * R, z: a Schnorr proof that the contributor knows d with delta1_after = d delta1_before -- R = k delta1_before for a fresh k,
 * c = zkr_mimcsponge_multihash(delta1_before.x, .y, delta1_after.x, .y, delta2_after.x.re, .x.im, .y.re, .y.im, R.x, R.y),
 * z = k + c d mod r.  Records chain by delta1_before == the previous record's delta1_after. */
#define ZKR_CONTRIBUTION_BYTES 352
/* key: a whole key (a shard: ZKR_ERR_ARG).  d32: 32 B LE, 1 < d < r, for reproducible tests; NULL draws d from the OS CSPRNG
 * inside the call.  Either way d, d^-1 and the Schnorr nonce are wiped from host and device memory before the call returns.
 * *out: a new, independent key on the same device (own arena and workspaces; every window level of C and H rebuilt from the new
 * base points, everything else carried over); `key` is left untouched and usable, so the caller can verify the pair.  Working
 * memory: the two keys and one compact arena; an allocation that does not fit fails with ZKR_ERR_HIP. */
int zkr_key_contribute(const zkr_key *key, const uint8_t *d32, zkr_key **out, uint8_t record_out[ZKR_CONTRIBUTION_BYTES]);
/* Host only (no GPU).  *valid = 1 iff every point of the record is on its curve and in its subgroup, none at infinity,
 * delta1_after != delta1_before, z < r, z delta1_before == R + c delta1_after, and e(delta1_after, g2) == e(g1, delta2_after);
 * zkr_last_error says what failed.  An error status only for a null pointer. */
int zkr_contribution_check(const uint8_t record[ZKR_CONTRIBUTION_BYTES], int *valid);
/* What a party that did NOT make the contribution runs on the key it was handed (both keys on one device).  *valid = 1 iff
 *   1. zkr_contribution_check(record);
 *   2. the record's delta1_before is `before`'s delta1, its delta1_after / delta2_after are `after`'s, and
 *      e(delta1_after, delta2_before) == e(delta1_before, delta2_after);
 *   3. same geometry, and the QAP sections, twiddles, rank maps, the A, B1 and B2 tables, alfa1, beta1, beta2 byte-identical;
 *   4. the window levels of `after`'s C and H tables are the multiples of its own base points (rebuilt from its compact arena
 *      and compared byte for byte; zkr_key_check level 1 only says that every stored point is on its curve);
 *   5. e(sum rho_s C'[s] + sum sigma_i H'[i], delta2_after) == e(sum rho_s C[s] + sum sigma_i H[i], delta2_before) for 128-bit
 *      rho_s, sigma_i from the OS CSPRNG (a wrong entry slips through with probability 2^-128), the sums by the keys' MSM path.
 * report (may be null): [0] = the first failed step (0: none), [1] = ZKR_KEYSEC_* of the first differing section (steps 3, 4).
 * ZKR_OK with *valid = 0 and a zkr_last_error line naming the step for a bad contribution; an error status only for bad
 * arguments (a shard, keys on different devices: ZKR_ERR_ARG) or a HIP failure. */
int zkr_key_contribution_verify(const zkr_key *before, const zkr_key *after, const uint8_t record[ZKR_CONTRIBUTION_BYTES], int *valid, uint64_t report[2]);
/* Host only.  The verifying key that goes with the contributed proving key: checks the record (zkr_contribution_check) and
 * that it continues THIS key (e(delta1_before, g2) == e(g1, vk_delta_2)), and returns a malloc'ed copy of vk_bin (zkr_free)
 * with vk_delta_2 (bytes 320..447) replaced by the record's delta2_after; ZKR_ERR_ARG otherwise. */
int zkr_vk_contribute(const void *vk_bin, size_t vk_len, const uint8_t record[ZKR_CONTRIBUTION_BYTES], void **vk_out, size_t *vk_out_len);

/* ---- a powers-of-tau transcript: the start of a key in which NO party knows t, alfa, beta -----------------------
 * A key from zkr_setup_r1cs is forgeable by whoever ran the setup: it knows t, alfa and beta, and a later delta contribution
 * does not take that away (the key publishes hExps[0] = Z(t)/delta G1 and the runner knows Z(t)).  The phase-1 transcript of
 * Bowe-Gabizon-Miers holds the powers a setup needs as GROUP ELEMENTS whose discrete logs are products of every contributor's
 * secrets, so they are unknown while ONE contributor forgot its share:
 *   ZKRPTAU1, power K (1..24), M = 2^K -- every coordinate 32 B LE standard form, G2 as x.re, x.im, y.re, y.im (as in vk_bin):
 *   32 B header: "ZKRPTAU1" | u32 K | u32 0 | u64 total length | 8 B zero
 *   tauG1 [2M] x 64 B (tau^i G1) | tauG2 [M] x 128 B (tau^i G2) | alfaTauG1 [M] x 64 B | betaTauG1 [M] x 64 B | betaG2 128 B
 * = 160 + 384 M bytes, in host memory; no point is ever infinity.  A transcript of power K serves every domain m <= M.
 * The record of a contribution (ZKR_PTAU_RECORD_BYTES), with tau1 = tauG1[1], alfa1 = alfaTauG1[0], beta1 = betaTauG1[0],
 * tau2 = tauG2[1], beta2 = betaG2:
 *   tau1_before | tau1_after | alfa1_before | alfa1_after | beta1_before | beta1_after (6 x 64) | tau2_after | beta2_after (2 x 128)
 *   | R_tau | R_alfa | R_beta (3 x 64) | z_tau | z_alfa | z_beta (3 x 32)
 * Three Schnorr proofs in the form of the delta record's: R = k before, z = k + c s mod r, accepted iff z before == R + c after,
 * with c = zkr_mimcsponge_multihash over a domain tag and the coordinates the proof binds (each point as x, y; G2 as 4 words):
 *   c_tau = H(1, tau1_before, tau1_after, tau2_after, R_tau), c_alfa = H(2, alfa1_before, alfa1_after, R_alfa),
 *   c_beta = H(3, beta1_before, beta1_after, beta2_after, R_beta). */
#define ZKR_PTAU_RECORD_BYTES 928
/* Host only: the transcript with tau = alfa = beta = 1 (every entry the generator of its group); malloc'ed, free with zkr_free. */
int zkr_ptau_new(unsigned power, void **ptau_out, size_t *ptau_len);
/* Multiplies tauG1[i], tauG2[i] by tau^i, alfaTauG1[i] by alfa tau^i, betaTauG1[i] by beta tau^i and betaG2 by beta, on the GPU
 * (one variable-base multiplication per point, each by a scalar of its own).  secrets96 = tau | alfa | beta, each 32 B LE with
 * 1 < s < r, for reproducible tests; NULL draws them from the OS CSPRNG inside the call.  Either way every copy of the secrets
 * the library holds in memory of its own -- the device table of powers, the device buffer of the ladders' unnormalised results,
 * the host staging, the Schnorr nonces and what z is formed from -- is wiped before the call returns.  Not within its reach: tau,
 * alfa and beta are handed to two small kernels by value, so they pass through the HIP runtime's kernel-argument buffers.  The input is checked
 * first (header and length; every coordinate canonical, every point finite and on its curve: ZKR_ERR_ARG otherwise).
 * *ptau_out: a new malloc'ed transcript (zkr_free); the input is left untouched.  No CPU fallback (ZKR_ERR_NO_DEVICE). */
int zkr_ptau_contribute(const void *ptau, size_t len, const uint8_t *secrets96, int device, void **ptau_out, size_t *out_len, uint8_t record_out[ZKR_PTAU_RECORD_BYTES]);
/* Host only.  records: n_records x ZKR_PTAU_RECORD_BYTES in the order the contributions were made.  *valid = 1 iff, for every
 * record, every point is on its curve and in its subgroup and none is infinity, each `after` differs from its `before`, each
 * z < r, the three Schnorr equations hold, e(tau1_after, g2) == e(g1, tau2_after) and the same for beta; and the records chain:
 * record 0's three `before` points are the G1 generator, record j + 1's `before` = record j's `after`.  zkr_last_error names the
 * record and the check that failed.  An error status only for a null pointer. */
int zkr_ptau_record_check(const uint8_t *records, size_t n_records, int *valid);
/* *valid = 1 iff every step holds; report (may be null): [0] = the first failed step (0: none), [1] = the vector it was found in
 * (0..4 in the layout's order):
 *   1. header and length are consistent (a failure here is ZKR_ERR_ARG: there is no transcript to speak of);
 *   2. every coordinate is canonical, every point finite and on its curve -- on the device, before any group arithmetic reads them;
 *   3. every G2 point has order r, [r] Q == O point by point (the twist's cofactor has small factors: a random combination
 *      would let a low-order component through with noticeable probability);
 *   4. tauG1[0] == G1 and tauG2[0] == G2;
 *   5. with 128-bit rho_i, sigma_i from the OS CSPRNG and the sums by the library's MSM path:
 *      e(sum rho_i tauG1[i+1], G2) == e(sum rho_i tauG1[i], tauG2[1]), i < 2M - 1;
 *      e(tauG1[1], S0) == e(G1, S1), S0 = sum_{i < M-1} sigma_i tauG2[i], S1 = sum_{i < M-1} sigma_i tauG2[i+1];
 *      e(sum_{i < M} sigma_i alfaTauG1[i], G2) == e(alfaTauG1[0], sum_{i < M} sigma_i tauG2[i]), the same for betaTauG1;
 *      e(betaTauG1[0], G2) == e(G1, betaG2);
 *   6. zkr_ptau_record_check(records), and the last record's `after` values are this transcript's tauG1[1], alfaTauG1[0],
 *      betaTauG1[0], tauG2[1], betaG2; n_records == 0 is accepted only for the all-generators transcript.
 * A bad transcript is ZKR_OK with *valid = 0 and a zkr_last_error line naming the step; a status below zero only for bad
 * arguments (step 1 included) or a HIP failure. */
int zkr_ptau_verify(const void *ptau, size_t len, const uint8_t *records, size_t n_records, int device, int *valid, uint64_t report[2]);
/* zkr_setup_r1cs with the transcript in the place of the toxic scalars: the key is, byte for byte, the key
 * zkr_setup_r1cs(r1cs, toxic = (tau, alfa, beta, 1, 1)) returns for the transcript's discrete logs -- which nobody knows -- and
 * vk_bin has vk_gamma_2 = vk_delta_2 = G2.  delta = 1 is public: the key is NOT sound before at least one zkr_key_contribute.
 * The domain m follows zkr_setup_r1cs's rule; m > 2^K is ZKR_ERR_ARG.  Steps 1-5 of zkr_ptau_verify run on the input first (a
 * failure of 2-5 is ZKR_ERR_BAD_KEY); the records are the caller's matter.  Derivation, all on the GPU: the Lagrange-basis points
 * of the first m entries of tauG1, tauG2, alfaTauG1, betaTauG1 by the inverse NTT over points; A[s], B1[s], B2[s] and
 * K[s] = sum polsA LagBeta + sum polsB LagAlfa + sum polsC Lag1 (C[s] above nPublic, IC[s] up to it) as sparse combinations of
 * them; hExps[i] = tauG1[i+m] - tauG1[i].  A table entry is dropped exactly when its point is infinity. */
int zkr_setup_r1cs_ptau(const void *r1cs_bin, size_t r1cs_len, const void *ptau, size_t ptau_len, int device, zkr_key **key_out, void **vk_out, size_t *vk_len);
/* Stage hooks, as zkr_ntt / zkr_msm_g1 are: n points in host memory, Montgomery affine as zkr_msm_g1 / g2 take them (64 B G1 /
 * 128 B G2 when g2 != 0; x == 0 encodes infinity), transformed in place.
 * zkr_points_scale_each: points[i] <- scalars[i] points[i], scalars 32 B LE standard form below r (ZKR_ERR_ARG otherwise).
 * zkr_group_ntt: the NTT of zkr_ntt with points for coefficients, n = 2^logn (logn 1..25), natural order in and out; the inverse
 * includes the factor 1 / n, so the inverse transform of tau^i G is the Lagrange-basis points L_j(tau) G of the domain. */
int zkr_points_scale_each(void *points_mont, const void *scalars_std, size_t n, int g2, int device);
int zkr_group_ntt(void *points_mont, unsigned logn, int inverse, int g2, int device);

/* ---- anybody: audit the finished key against circuit, transcript and records alone (snarkjs users: `zkey verify`) ----------
 * Host only.  For delta records what zkr_ptau_record_check is for phase-1 records: records = n_records x ZKR_CONTRIBUTION_BYTES
 * in the order the contributions were made; *valid = 1 iff every record passes zkr_contribution_check, record 0's delta1_before
 * is the G1 generator (a key from a transcript starts at delta = 1) and record j + 1's delta1_before is record j's delta1_after.
 * zkr_last_error names the record and the check.  n_records == 0 is valid.  An error status only for a null pointer. */
int zkr_contribution_chain_check(const uint8_t *records, size_t n_records, int *valid);
/* What a depositor, an exchange or whoever deploys the verifier runs.  It holds the public artefacts only -- the circuit (cs), the
 * phase-1 transcript with its records, the delta records, the proving key and vk_bin -- no intermediate key, and it repeats
 * nothing of the setup's derivation: the setup goes through NTTs over points, the audit through random combinations on the scalar
 * side.  Notation: n, p, m the key's nVars, nPublic and domain; polsA / polsB the key's QAP sides with the p + 1
 * rows the setup appends to A, polsC the system's third side (zero on those rows); for a vector v over the signals
 * x(v) = iNTT_m(j -> sum_s polsX[s][j] v_s), so that sum_s v_s X_s(tau) = sum_i x(v)_i tau^i; T(v) = sum_i a(v)_i betaTauG1[i] +
 * b(v)_i alfaTauG1[i] + c(v)_i tauG1[i].  rho_s (s < n), sigma_i (i < m): 128 bits each from the OS CSPRNG; rho_pub / rho_priv:
 * rho on the signals 0..p / above p, zero elsewhere.  A wrong entry slips through with probability 2^-128.  Every sum runs on the
 * device through the MSM path the prover uses; the pairings on the host.
 * Steps, in order; the first failure ends the call:
 *   1. the transcript passes zkr_ptau_verify's steps 2-6 with ptau_records;
 *   2. m <= 2^K, and zkr_r1cs_matches_key(cs, key);
 *   3. zkr_contribution_chain_check(delta_records), and the key's delta1 / delta2 are the last record's delta1_after /
 *      delta2_after -- with no records, the generators;
 *   4. the key's alfa1 == alfaTauG1[0], beta1 == betaTauG1[0], beta2 == betaG2; vk_alfa_1 and vk_beta_2 are the same transcript
 *      entries; vk_gamma_2 == G2; vk_delta_2 == the key's delta2;
 *   5. the key's two twiddle sections are the tables of its domain, and the window levels of all five tables are the multiples
 *      of their own base points: each rebuilt and compared byte for byte, one table at a time (as step 4 of
 *      zkr_key_contribution_verify does for C and H).  The sums below read those levels.  The twiddles are bytes of the key
 *      file, which a load does not check (zkr_key_check level 1 does): the audit's own transforms use tables built for the call;
 *   6. E1 sum_s rho_s A[s] == sum_i a(rho)_i tauG1[i];  E2 sum_s rho_s B1[s] == sum_i b(rho)_i tauG1[i];
 *      E3 sum_s rho_s B2[s] == sum_i b(rho)_i tauG2[i];
 *   7. E4 sum_{s<=p} rho_s IC[s] == T(rho_pub): the verifying key's IC points, which go on chain (gamma = 1);
 *   8. E5 e(sum_{s>p} rho_s C[s], delta2) == e(T(rho_priv), G2) and E6 e(sum_i sigma_i hExps[i], delta2) ==
 *      e(sum_i sigma_i (tauG1[i+m] - tauG1[i]), G2), in one pairing product.  A table entry the key dropped because it is the
 *      point at infinity adds nothing on the left; the right side must then agree by itself.  This is the statement about the
 *      key's C query that zkr_r1cs_matches_key cannot make.
 * report (may be null): [0] the first failed step (0: none); [1] a detail -- the record's index for step 3; for steps 5 and 6 the
 * first table that differs (0 A, 1 B1, 2 B2, 3 C, 4 hExps; 5 at step 5: the twiddles); else 0; [2] the number of phase-1 records;
 * [3] the number of delta records.
 * A KEY WITH report[3] == 0 IS CONSISTENT AND NOT SOUND: delta = 1 is public, and whoever knows delta forges proofs.  A key is
 * sound if one phase-1 contributor and one delta contributor forgot their secrets; the audit says that the records are about this
 * key, not who the contributors were.
 * The key's evaluation-form side tables (zkr_key_eval_tables) are not part of the audit: whoever proves derives them locally from
 * the points audited here.
 * A key that fails is ZKR_OK with *valid = 0 and a zkr_last_error line that says "step N".  A status below zero only for bad
 * arguments or a HIP failure: a null pointer, a shard, key and system on different devices are ZKR_ERR_ARG; so are -- before any
 * device call -- a malformed transcript header or length, a vk_len that does not match its IC count, and an IC count other than
 * p + 1.  The key is only read: nothing is cached on it.  Working memory above the key: the transcript's body; 18 m + 3 n scalars;
 * one table at a time -- in step 5 a copy of the key's largest table, in the sums one vector's window levels with one MSM
 * workspace. */
int zkr_key_audit(const zkr_key *key, zkr_r1cs *cs, const void *ptau, size_t ptau_len, const uint8_t *ptau_records, size_t n_ptau_records,
                  const uint8_t *delta_records, size_t n_delta_records, const void *vk_bin, size_t vk_len, int *valid, uint64_t report[4]);

/* Circuit shape drawn by the zkr_synth_* calls of the CALLING THREAD (thread-local, default 0): 0 = rollup-shaped (default; 1-3 terms
 * per row, 3 % boolean and 2 % small signals, a third of the signals absent from B), 1 = dense random (BASELINE.json
 * configs[4]: every row is (4 random signals) x (4 random signals) = new signal; no infinity points in any query). */
int zkr_synth_set_shape(unsigned shape);
void zkr_free(void *p);

/* ---- the reference's rollup circuit without circom / snarkjs (host only) ---- */
/* Witness-side crypto of operator/src/utils/crypto.ts.  Field elements are 32 B little-endian, standard form.
 * zkr_mimcsponge_multihash = multiHash (crypto.ts:28-30; MiMCSponge-220, key 0, one output; operands taken mod r);
 * zkr_babyjub_pubkey = genPublicKey (crypto.ts:78-84, including formatPrivKeyForBabyJub :58-76), pub = x | y;
 * zkr_eddsa_sign = sign (crypto.ts:143-168) over n message elements, sig = R8x | R8y | S;
 * zkr_eddsa_verify = verify (crypto.ts:170-177), *valid = 0 / 1. */
int zkr_mimcsponge_multihash(const uint8_t *in, size_t n, uint8_t out[32]);
int zkr_babyjub_pubkey(const uint8_t priv[32], uint8_t pub[64]);
int zkr_eddsa_sign(const uint8_t priv[32], const uint8_t *msg, size_t n, uint8_t sig[96]);
int zkr_eddsa_verify(const uint8_t *msg, size_t n, const uint8_t sig[96], const uint8_t pub[64], int *valid);
/* The same hash batch-parallel on the GPU (one thread per hash): out[t] = multiHash(inputs[t * arity .. + arity)), host
 * buffers, standard form; and the reference's balance tree (operator/src/utils/merkletree.ts:44-83, hashLeftRight of
 * adjacent pairs) built level by level on the device: leaves = 2^depth x 32 B, levels_out = all levels concatenated,
 * leaves first, root last ((2^(depth+1) - 1) x 32 B).  No CPU fallback (ZKR_ERR_NO_DEVICE). */
int zkr_mimcsponge_multihash_batch(const void *inputs_std, size_t count, unsigned arity, void *out_std, int device);
int zkr_balance_tree_build(const void *leaves_std, unsigned depth, void *levels_out, int device);
/* BatchProcessTx(batch, depth) (prover/circuits/batchprocesstx.circom:3-75; `tx.circom` = (2, 6)) as a rank-1
 * constraint system in the r1cs_bin layout of zkr_setup_r1cs, and its witness builder -- the counterpart of
 * `compiler(tx.circom)` + `Circuit.calculateWitness` (operator/src/snarks/common.ts:12-17).  Public signals keep
 * circom's order: newBalanceTreeRoot, then balanceTreeRoot[batch], txData[batch][8], txSenderPublicKey[batch][2],
 * txSenderBalance[batch], txSenderNonce[batch], txSenderPathElements[batch][depth], txRecipientPublicKey[batch][2],
 * txRecipientBalance[batch], txRecipientNonce[batch], txRecipientPathElements[batch][depth],
 * intermediateBalanceTreeRoot[batch], intermediateBalanceTreePathElements[batch][depth]  (73 for (2, 6)).
 * zkr_rollup_witness takes the n_public - 1 inputs in that order (32 B each) and returns the full witness
 * (nVars x 32 B, the buffer binarifyWitness would produce; free with zkr_free); inputs that violate the circuit fail
 * with ZKR_ERR_UNSATISFIED and a message naming the first violated statement.  The constraint system is this build's
 * own formulation of the circuit (see csrc/rollup.cpp): its keys come from zkr_setup_r1cs, not from a circom build. */
/* Withdraw() (prover/circuits/withdraw.circom:4-25): public signals publicKey[0], publicKey[1], nullifier; the private
 * input is the FORMATTED key, zkr_babyjub_format_privkey = formatPrivKeyForBabyJub (crypto.ts:58-76), as in
 * prover/__tests__/withdraw.test.ts:22-25.  Same conventions as the two calls below. */
int zkr_babyjub_format_privkey(const uint8_t priv[32], uint8_t out[32]);
int zkr_withdraw_r1cs(void **r1cs_bin, size_t *r1cs_len);
int zkr_withdraw_witness(const uint8_t private_key[32], const uint8_t nullifier[32], void **witness_bin, size_t *witness_len);
int zkr_rollup_info(uint32_t batch, uint32_t depth, uint32_t *n_vars, uint32_t *n_public, uint32_t *n_constraints);
int zkr_rollup_r1cs(uint32_t batch, uint32_t depth, void **r1cs_bin, size_t *r1cs_len);
int zkr_rollup_witness(uint32_t batch, uint32_t depth, const uint8_t *inputs, size_t n_inputs, void **witness_bin, size_t *witness_len);
/* The same for MANY rollup batches at once, ON THE GPU (one thread per transaction): inputs = n_batches x n_inputs x 32 B
 * (host memory), d_witnesses = device memory for n_batches x nVars x 32 B, each witness laid out as zkr_rollup_witness returns
 * it (byte for byte) and ready for zkr_prove_batch_device -- `Circuit.calculateWitness` (operator/src/snarks/common.ts:15-17)
 * for a queue of batches without touching the host cores.  ZKR_ERR_UNSATISFIED names the first batch / transaction /
 * statement that fails; ZKR_ERR_ARG an input that is not below r.  No CPU fallback (ZKR_ERR_NO_DEVICE). */
int zkr_rollup_witness_batch_device(uint32_t batch, uint32_t depth, const uint8_t *inputs, size_t n_inputs, size_t n_batches, void *d_witnesses, int device);
/* Test hook: the program one GPU thread runs per transaction (csrc/rollup_witness.hpp), run on the HOST for one batch --
 * witness_out = nVars x 32 B as zkr_rollup_witness lays it out, *stmt = code of the first violated statement (0: none;
 * zkr_rollup_statement_text gives its wording), *tx = its transaction.  Lets the CPU suite compare the GPU builder's program
 * with the host builder signal for signal. */
int zkr_rollup_witness_program_host(uint32_t batch, uint32_t depth, const uint8_t *inputs, size_t n_inputs, uint8_t *witness_out, uint32_t *stmt, uint32_t *tx);
const char *zkr_rollup_statement_text(uint32_t stmt);
/* zkr_rollup_witness_batch_device with the inputs already in device memory (same kernels, same errors, same bytes): d_inputs =
 * n_batches x n_inputs x 32 B as zkr_ledger_sequence leaves them.  The kernels run on `stream` (NULL: the default stream), the
 * one the inputs were written on; the call returns when the witnesses are complete. */
int zkr_rollup_witness_batch_from_device(uint32_t batch, uint32_t depth, const void *d_inputs, size_t n_inputs, size_t n_batches,
                                         void *d_witnesses, int device, void *stream);

/* ---- the user's side of crypto.ts and the withdraw circuit in bulk ON THE GPU, one thread per item (csrc/zkr_wallet.hip over
 * csrc/wallet_program.hpp): formatPrivKeyForBabyJub (crypto.ts:58-76), genPublicKey (:78-84) and sign (:143-168)
 * for n keys, each item equal to zkr_babyjub_format_privkey / zkr_babyjub_pubkey / zkr_eddsa_sign bit for bit.  privs: n x 32 B,
 * msgs: n x arity x 32 B, arity 1..64; out: n x 32 B, pubs: n x 64 B, sigs: n x 96 B (R8x R8y S); all standard form.
 * Arguments are checked first, without a device: a null pointer or an arity out of range is ZKR_ERR_ARG, and so is a key or a
 * message element not below r, with the first such item's index in zkr_last_error (what the host calls refuse).  Then the
 * device: no CPU fallback (ZKR_ERR_NO_DEVICE).  n = 0 is ZKR_OK with nothing launched.  On an error return the outputs are
 * untouched.  Any n: more than 2^20 items go to the device in pieces.  Every device buffer that held a key or a formatted
 * scalar is zeroed before it is freed.  The kernels are NOT constant time. */
int zkr_babyjub_format_privkey_batch(const uint8_t *privs, size_t n, uint8_t *out, int device);
int zkr_babyjub_pubkey_batch(const uint8_t *privs, size_t n, uint8_t *pubs, int device);
int zkr_eddsa_sign_batch(const uint8_t *privs, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *sigs, int device);
/* `Circuit.calculateWitness` for withdraw.circom (operator/src/snarks/withdraw.ts:6-10) for n withdrawals at once: private_keys
 * (FORMATTED keys) and nullifiers are n x 32 B in host memory, d_witnesses = device memory for n x nVars x 32 B, each witness
 * laid out as zkr_withdraw_witness returns it (byte for byte) and ready for zkr_prove_batch_device, zkr_r1cs_check_device and
 * zkr_verify_each_device.  The kernels run on `stream` (NULL: the default stream); the call returns when the witnesses are
 * complete.  An input not below r is ZKR_ERR_ARG (checked before the device); a key past 253 bits is ZKR_ERR_UNSATISFIED naming
 * the first failing witness and the statement, found before anything is launched.  No CPU fallback (ZKR_ERR_NO_DEVICE). */
int zkr_withdraw_witness_batch_device(const uint8_t *private_keys, const uint8_t *nullifiers, size_t n, void *d_witnesses, int device, void *stream);
/* Test hooks: the programs one GPU thread runs per item (csrc/wallet_program.hpp), run on the HOST for one item.  pubkey:
 * formatted = the scalar of zkr_babyjub_format_privkey, pub = zkr_babyjub_pubkey's; sign: sig = zkr_eddsa_sign's; withdraw:
 * *stmt = code of the first violated statement (zkr_withdraw_statement_text gives its wording) with witness_out untouched, or
 * 0 with witness_out = nVars x 32 B as zkr_withdraw_witness lays it out (zkr_withdraw_n_vars: nVars). */
int zkr_wallet_pubkey_program_host(const uint8_t priv[32], uint8_t formatted[32], uint8_t pub[64]);
int zkr_wallet_sign_program_host(const uint8_t priv[32], const uint8_t *msg, unsigned arity, uint8_t sig[96]);
int zkr_withdraw_witness_program_host(const uint8_t private_key[32], const uint8_t nullifier[32], uint8_t *witness_out, uint32_t *stmt);
const char *zkr_withdraw_statement_text(uint32_t stmt);
uint32_t zkr_withdraw_n_vars(void);

/* ---- the rest of crypto.ts: key agreement and the MiMC7 cipher (csrc/zkr_crypto.hip over csrc/crypto_program.hpp).
 * All values 32 B little-endian standard form.  One item on the host, no device needed:
 *   zkr_mimc7_round_constants  circomlib mimc7.js getConstants("mimc", 91): 91 x 32 B, c_0 = 0
 *   zkr_mimc7_hash             mimc7.hash(x, k)
 *   zkr_mimc7_multihash        mimc7.multiHash(in[0..n), key)
 *   zkr_babyjub_ecdh           ecdh(priv, pub) (crypto.ts:86-93): the x coordinate of formatPrivKeyForBabyJub(priv) * pub
 *   zkr_mimc7_encrypt          encrypt(msg, key) (crypto.ts:95-110): *iv = multiHash(msg, 0), out[i] = msg[i] + hash(key, iv + i) --
 *                              the INTEGER sum, below 2r, as the reference's BigInt `+` leaves it [DEP-KNOWLEDGE]
 *   zkr_mimc7_decrypt          decrypt({iv, msg}, key) (crypto.ts:112-123): (enc[i] - hash(key, iv + i)) mod r for enc[i] < 2r
 * ecdhEncrypt / ecdhDecrypt (crypto.ts:125-141) are zkr_babyjub_ecdh followed by zkr_mimc7_encrypt / zkr_mimc7_decrypt.
 * ZKR_ERR_ARG, naming the item (0 for these calls) and the element: a key, message element, iv or public-key coordinate not below
 * r; a ciphertext element not below 2r; a public key that is not on the curve (the reference multiplies whatever it is given:
 * a stated deviation); an arity outside 1..65536.  The identity and the low-order points are accepted, as in the reference. */
int zkr_mimc7_round_constants(uint8_t *out);
int zkr_mimc7_hash(const uint8_t x[32], const uint8_t k[32], uint8_t out[32]);
int zkr_mimc7_multihash(const uint8_t *in, size_t n, const uint8_t key[32], uint8_t out[32]);
int zkr_babyjub_ecdh(const uint8_t priv[32], const uint8_t pub[64], uint8_t shared[32]);
int zkr_mimc7_encrypt(const uint8_t key[32], const uint8_t *msg, unsigned arity, uint8_t iv[32], uint8_t *out);
int zkr_mimc7_decrypt(const uint8_t key[32], const uint8_t iv[32], const uint8_t *enc, unsigned arity, uint8_t *out);
/* The same for whole lists ON THE GPU, each item equal to the host call's bit for bit: one thread per key pair (ecdh), per message
 * (the iv) and per message ELEMENT (the keystream).  privs, keys, ivs, shared: n x 32 B; pubs: n x 64 B; msgs, encs, out: n x arity
 * x 32 B, one arity for the whole call.  In the ecdh_* calls the shared keys never leave the device.  The refusals above come
 * first and without a device, naming the first offending item; then no CPU fallback (ZKR_ERR_NO_DEVICE).  n = 0 is ZKR_OK with
 * nothing launched.  On an error return the outputs are untouched.  Every device buffer that held a key or a plaintext is zeroed
 * before it is freed.  The kernels are NOT constant time. */
int zkr_babyjub_ecdh_batch(const uint8_t *privs, const uint8_t *pubs, size_t n, uint8_t *shared, int device);
int zkr_mimc7_encrypt_batch(const uint8_t *keys, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *ivs, uint8_t *out, int device);
int zkr_mimc7_decrypt_batch(const uint8_t *keys, const uint8_t *ivs, const uint8_t *encs, unsigned arity, size_t n, uint8_t *out, int device);
int zkr_ecdh_encrypt_batch(const uint8_t *privs, const uint8_t *pubs, const uint8_t *msgs, unsigned arity, size_t n, uint8_t *ivs, uint8_t *out, int device);
int zkr_ecdh_decrypt_batch(const uint8_t *privs, const uint8_t *pubs, const uint8_t *ivs, const uint8_t *encs, unsigned arity, size_t n, uint8_t *out, int device);

/* ---- the operator's ledger on the GPU: a queue of signed transactions -> a status each and the circuit inputs of every whole
 * batch, in device memory (csrc/zkr_sequencer.hip).  Stands in for the per-transaction loop of
 * operator/src/routes/send.ts:72-135 and the tree updates of operator/src/routes/pubsub.ts:19-66.  The ledger holds the account
 * records (host) and the whole balance tree (device, 2^(depth+1) - 1 nodes).  No CPU fallback (ZKR_ERR_NO_DEVICE). ---- */
typedef struct zkr_ledger zkr_ledger;
int zkr_ledger_new(unsigned depth, int device, zkr_ledger **out); /* empty tree, zero leaves; depth 1..24 */
void zkr_ledger_free(zkr_ledger *l);
/* onEventUpdateMerkleTree (pubsub.ts:19-66): insert (index == accounts so far) or overwrite (index below it); an index above it
 * is ZKR_ERR_ARG ("out of sync").  records: n x 4 x 32 B  pubX pubY balance nonce, standard form; every element below r, balance
 * and nonce below 2^250 (the circuit's range checks), ZKR_ERR_ARG otherwise.  A refused call leaves the ledger as it was. */
int zkr_ledger_deposit(zkr_ledger *l, const uint32_t *indices, const uint8_t *records, size_t n);
int zkr_ledger_info(const zkr_ledger *l, uint64_t out[4]); /* depth, accounts, transactions applied, batches emitted */
int zkr_ledger_root(const zkr_ledger *l, uint8_t root[32]);
int zkr_ledger_account(const zkr_ledger *l, uint32_t index, uint8_t record[128], uint8_t *path /* depth x 32 B, may be NULL */);
/* verify (crypto.ts:170-177) for n signatures at once, one verdict byte each; equals zkr_eddsa_verify bit for bit.  msgs: n x
 * arity x 32 B (elements of any size are taken mod r, as zkr_mimcsponge_multihash takes them), sigs: n x 96 B, pubs: n x 64 B. */
int zkr_eddsa_verify_batch(const uint8_t *msgs, unsigned arity, const uint8_t *sigs, const uint8_t *pubs, size_t n, uint8_t *verdicts, int device);
/* txs: n_txs x 8 x 32 B, the txData row of batchprocesstx.circom (from to amount fee nonce R8x R8y S).
 * status: n_txs bytes.  d_inputs: device memory for (n_txs / batch) x (n_public - 1) x 32 B.
 * *n_batches: batches written.  *consumed: transactions decided (the caller resubmits txs[consumed..]).
 *
 * The queue is gone through in order against the ledger's state.  A status is the first rule of this list the transaction
 * breaks, 0 = accepted:
 *    1  `from` is an account of the ledger (send.ts:76)          2  `to` is an account of the ledger (send.ts:82)
 *    3  every element is below r; amount, fee and nonce are below 2^250
 *    4  amount > 0                                                5  fee > 0
 *    6  sender balance > amount + fee (the circuit's strict comparison; send.ts:91 is laxer, what it admits beyond cannot be proved)
 *    7  fee >= (amount div 1000) * 3 (send.ts:101)                8  nonce = sender's nonce + 1 (send.ts:112)
 *    9  the recipient's new balance stays below 2^250
 *   10  the signature over multiHash([from, to, amount, fee, nonce]) verifies under the sender's stored key, as the circuit
 *       checks it (a key whose order divides 8 fails here)
 * With A transactions accepted in the whole queue only the first A - (A mod batch) of them are applied; *consumed is the position
 * just behind the last of them, and every transaction from there on has status 255 ("not reached").  Batch b's inputs are those
 * of its `batch` applied transactions in the order zkr_rollup_witness takes them.  Everything runs on `stream` (NULL: the default
 * stream); the call returns when the statuses are final and d_inputs is complete.  On any error return the ledger is unchanged. */
int zkr_ledger_sequence(zkr_ledger *l, const uint8_t *txs, size_t n_txs, uint32_t batch, uint8_t *status, void *d_inputs,
                        size_t *n_batches, size_t *consumed, void *stream);
/* Wall milliseconds of the last zkr_ledger_sequence (or zkr_ledger_replay*) call's stages -- signatures, host pass, leaf hashes,
 * tree levels, assembly -- recorded only while the environment variable ZKR_SEQUENCER_STAGES is set (the call then waits for the
 * stream after each stage).  For a replay the first slot also holds the signals' way to the device or back from it, the last one
 * the comparison and the store. */
int zkr_ledger_stage_times(const zkr_ledger *l, double ms[5]);

/* ---- following the chain: RollUp.sol:81-161 for a run of consecutive published batches, against the ledger's state (DESIGN.md
 * 9g).  Every input of BatchProcessTx is public (batchprocesstx.circom:12-34), so the public signals of a batch are its complete
 * state transition: a restarted operator rebuilds its ledger from them, and a second party follows the state and checks that each
 * batch starts from the current root and ends in the root it claims.  zkr_ledger_sequence WRITES the signals the ledger derives;
 * a replay COMPARES published signals with them and says, per batch, where they first differ.
 * publics_std: n_batches x nPublic x 32 B in host memory, standard form, circom's order (newBalanceTreeRoot, then the inputs as
 *   zkr_ledger_sequence writes them); nPublic = 1 + batch * (18 + 3 * depth).
 * proof_verdicts: NULL, or n_batches bytes as zkr_verify_each returns them (non-zero = the contract would revert, RollUp.sol:96).
 *   Proofs are not verified inside the call: the caller composes zkr_verify_each.
 * flags: ZKR_REPLAY_SIGNATURES = also check every transaction's signature under the sender's stored key (rule 10 of
 *   zkr_ledger_sequence, the same kernel).
 * verdicts: n_batches bytes.  where: n_batches words.  *applied: batches applied = index of the first refused batch, or n_batches.
 *
 * Batches are judged in order, each against the state all earlier ones leave.  The first batch with a non-zero verdict keeps it
 * and every later one is 255; the ledger ends as it stands after the last batch with verdict 0 (records, tree, root and the
 * counters of zkr_ledger_info).  A batch gets the first of these codes that holds:
 *    1  it cannot be applied: a signal not below r; `from` / `to` no account; amount, fee or nonce not below 2^250; a sender
 *       balance below amount + fee; a recipient balance that would reach 2^250.  where = the offending signal (the lowest one not
 *       below r, else the first transaction's; for the balances the transaction's amount signal, 1 + batch + 8k + 2)
 *    2  balanceTreeRoot[0] is not the ledger's root before the batch (RollUp.sol:92).  where = 1
 *    3  proof_verdicts[b] != 0 (RollUp.sol:96).  where = 0
 *    5  only with ZKR_REPLAY_SIGNATURES: a signature fails under the sender's stored key.  where = the transaction within the batch
 *    4  some signal differs from what the ledger derives from txData and its own state.  where = the lowest differing signal
 *       (0 = newBalanceTreeRoot)
 *    0  applied.  where = 0
 * The arithmetic is the contract's (RollUp.sol:118-158) and processtx.circom's, from == to included: the sender's leaf moves first
 * (balance - amount - fee, nonce := the transaction's), then the recipient's (balance + amount).  Rules 4-8 of zkr_ledger_sequence
 * (positive amount and fee, the strict balance, the fee floor, nonce + 1) are NOT applied: they are operator policy or the
 * circuit's matter (code 3); the contract applies whatever was proved, and a follower has to track the contract.  Fees are not
 * accounted (accuredFees), events and calldata are not decoded.
 * An argument error (null, batch 0, a geometry zkr_rollup_info refuses, more than 2^22 transactions, a null witness pointer) is
 * ZKR_ERR_ARG and leaves the ledger, verdicts and where untouched and *applied = 0.  No CPU fallback (ZKR_ERR_NO_DEVICE). ---- */
#define ZKR_REPLAY_SIGNATURES 1u
int zkr_ledger_replay(zkr_ledger *l, const void *publics_std, size_t n_batches, uint32_t batch, const uint8_t *proof_verdicts,
                      uint32_t flags, uint8_t *verdicts, uint32_t *where, size_t *applied, void *stream);
/* The same with the signals read in place: d_witnesses_std is a host array of n_batches device pointers on the ledger's device,
 * batch b's signals are words 1..nPublic of witness b (the convention of zkr_verify_each_device); no other word is read. */
int zkr_ledger_replay_device(zkr_ledger *l, const void *const *d_witnesses_std, size_t n_batches, uint32_t batch,
                             const uint8_t *proof_verdicts, uint32_t flags, uint8_t *verdicts, uint32_t *where, size_t *applied,
                             void *stream);
/* host only */
/* Test hook: the host pass of zkr_ledger_replay alone (verdict 1 and the arithmetic), as zkr_sequence_plan_host is for the
 * sequencer.  verdicts[b] = 0 planned, 1 the first batch that cannot be applied (where[b] = its signal), 255 behind it; *planned =
 * that batch's index or n_batches.  With T = *planned x batch: idx (may be NULL) 2T leaf indices, old_rec / new_rec (may be NULL)
 * 2T x 128 B, prev (may be NULL) the three tables [3][depth][2T]; room for 2 x batch x n_batches updates each. */
int zkr_replay_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const void *publics_std, size_t n_batches,
                         uint32_t batch, uint8_t *verdicts, uint32_t *where, size_t *planned, uint32_t *idx, uint8_t *old_rec,
                         uint8_t *new_rec, int32_t *prev);
/* Test hook: the host pass of zkr_ledger_sequence (rules 1-9 and the arithmetic; rule 10 from sig_verdicts, one byte per
 * transaction) over records = n_accounts x 128 B.  prev (may be NULL): int32 [3][depth][2T], T = the number of status-0
 * transactions, room for 3 x depth x 2 x n_txs: table 0 [l][u] = the latest update u' < u under the sibling of update u's node
 * of level l, or -1 (the stored node); table 1 [l][2k] the same for the recipient's node asked before update 2k (odd entries
 * -1); table 2 [l][u] = 1 when update u holds the last version of its node of level l.  Update 2k is transaction k's sender
 * leaf, 2k + 1 its recipient leaf. */
int zkr_sequence_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *txs, size_t n_txs,
                           const uint8_t *sig_verdicts, uint32_t batch, uint8_t *status, size_t *consumed, int32_t *prev);

/* ---- keeping the ledger: read-out, snapshots with a checked restore, checkpoints with rollback, and an audit of the stored tree
 * (DESIGN.md 9h).  Stands in for the load / save of operator/src/utils/merkletree.ts:274-403 around every event (pubsub.ts:35,65),
 * which trusts the root it stored.  All device work runs under the ledger's lock on the default stream and every call returns
 * synchronised.  None of these calls changes what an earlier call returns; with no checkpoint open zkr_ledger_deposit,
 * zkr_ledger_sequence and the replays launch what they launched before.
 *
 * Read-out.  zkr_ledger_records copies `count` records of 128 B (pubX pubY balance nonce) from `first` on; a range past the
 * accounts is ZKR_ERR_ARG.  zkr_ledger_tree gives the device address and byte length of the stored tree, (2^(depth+1) - 1) x 32 B,
 * leaves first, root last (the layout of zkr_balance_tree_build), as zkr_key_arena gives a key's arena: a read-only view, valid
 * until zkr_ledger_free; its contents move with every state-changing call.
 *
 * Snapshot "ZKRLEDG1", 128 + 128 x accounts bytes, integers little-endian, field elements 32 B standard form:
 *     0  "ZKRLEDG1"      8  u32 depth     12  u32 0      16  u64 accounts     24  u64 applied     32  u64 batches     40  24 B zero
 *    64  root           96  tag = zkr_mimcsponge_multihash(depth, accounts, applied, batches, root)          128  the records
 * The tag covers the header, the root covers the records once they are rebuilt: no byte is unprotected.  Checkpoints are not part
 * of a snapshot; it is the current state.
 * zkr_ledger_snapshot returns a malloc'ed blob (zkr_free).  zkr_ledger_save writes it to `path`.tmp and renames that to `path`: a
 * crash leaves the old file or the new one.
 * zkr_ledger_snapshot_check (host only) checks magic, reserved words, length, depth 1..24, accounts <= 2^depth, the tag, and that
 * every element is below r and every balance and nonce below 2^250 (what zkr_ledger_deposit requires).  *valid = 0 comes with
 * ZKR_OK and a zkr_last_error line naming the first failure; info = depth, accounts, applied, batches of a valid blob.
 * zkr_ledger_restore / zkr_ledger_load_file: that check first -- a failure is ZKR_ERR_ARG, reported before the device is looked
 * at; then the device (ZKR_ERR_NO_DEVICE, no CPU fallback); then a new ledger whose tree is built in bulk from the records: leaf
 * hashes straight into the tree, one launch per level over the nodes whose subtree holds an account, fewer than 2 x accounts +
 * depth hashes and no tables (records go up in pieces of at most 2^20).  The rebuilt root is read back and compared with the
 * blob's: a mismatch is ZKR_ERR_BAD_KEY with both roots in zkr_last_error, and no ledger is returned.  The counters are the blob's.
 *
 * Checkpoints.  zkr_ledger_checkpoint opens one and returns its id; they nest.  While at least one is open every storing call
 * (zkr_ledger_deposit, zkr_ledger_sequence, both replays) first copies (node, old value) of every tree node it is about to
 * overwrite into a journal the ledger owns, and the old records and counters beside it.  zkr_ledger_rollback(id) puts the ledger
 * back exactly as it stood at zkr_ledger_checkpoint(id) -- records, account count (accounts inserted since disappear), every byte
 * of the stored tree, applied and batches -- discards every checkpoint taken after `id`, and leaves `id` open: it can be rolled
 * back to again.  zkr_ledger_release(id) forgets the marker and changes no state; with the last marker the journal is emptied
 * and nothing more is recorded.  An unknown, released or discarded id is ZKR_ERR_ARG.  A journal that cannot grow is ZKR_ERR_HIP,
 * raised before anything is stored: "on any error return the ledger is unchanged" covers the journal too.
 * zkr_ledger_journal_info: out = open checkpoints, journalled nodes.
 *
 * zkr_ledger_audit is the ledger's zkr_key_check: one launch over all nodes, each check from stored values alone.  Leaf i <
 * accounts must be the leaf hash of record i; a node whose whole subtree lies past the last account must be its level's
 * empty-subtree constant (compared, not hashed); every other inner node must be the hash of its two stored children; a stored
 * word not below r is a difference.  A bad tree is ZKR_OK with *sound = 0 and report = (level, index) of the first bad node,
 * lowest level first, then lowest index; a sound one *sound = 1 and report = (0, 0). ---- */
int zkr_ledger_records(const zkr_ledger *l, size_t first, size_t count, uint8_t *out);
int zkr_ledger_tree(const zkr_ledger *l, const void **dev_ptr, size_t *len);
int zkr_ledger_snapshot(const zkr_ledger *l, void **blob, size_t *len);
int zkr_ledger_save(const zkr_ledger *l, const char *path);
int zkr_ledger_snapshot_check(const void *blob, size_t len, uint64_t info[4], int *valid);
int zkr_ledger_restore(const void *blob, size_t len, int device, zkr_ledger **out);
int zkr_ledger_load_file(const char *path, int device, zkr_ledger **out);
int zkr_ledger_checkpoint(zkr_ledger *l, uint64_t *id);
int zkr_ledger_rollback(zkr_ledger *l, uint64_t id);
int zkr_ledger_release(zkr_ledger *l, uint64_t id);
int zkr_ledger_journal_info(const zkr_ledger *l, uint64_t out[2]);
int zkr_ledger_audit(zkr_ledger *l, uint64_t report[2], int *sound);

/* ---- the ledger's book: the contract's side of the ledger, by public key (csrc/zkr_book.hip).  RollUp.sol addresses
 * accounts by hashPair(publicKey) and keeps what goes with that -- balanceTreeUsers / isPublicKeysRegistered (RollUp.sol:56-57),
 * usedNullifiers (:58), accuredFees (:63).  zkr_ledger_deposit takes the EVENT the contract emits after that work; a book takes the
 * CALLS.  A ledger without an open book behaves and launches exactly as before.  No CPU fallback (ZKR_ERR_NO_DEVICE); every
 * by-key call on a ledger with no open book is ZKR_ERR_ARG; argument checks run before the device is looked at; n is at most
 * 2^22 per call and n = 0 is an empty result.  All device work runs under the ledger's lock and every call returns synchronised.
 * On any error return the ledger and the book are unchanged.
 *
 * State, all on the ledger's device.  Key table: hashPair(pubX, pubY) of every record (one MiMCSponge multiHash of two elements
 * per account) and an open-addressing table of 2^(depth+1) slots over them (load factor at most 1/2), built from the ledger's
 * RECORDS and nothing else; where two accounts hold one key (the contract cannot produce that, zkr_ledger_deposit can) the lowest
 * index owns it.  zkr_ledger_deposit on a ledger with an open book marks the table stale when it writes a key that differs from
 * the stored one or inserts an account, zkr_ledger_rollback marks both tables stale; a stale table is rebuilt at the next by-key
 * call.  zkr_ledger_sequence and the replays never move keys.  Nullifier set: the nullifiers in acceptance order and a slot table
 * of 2^nullifier_cap_log2 slots (default 10, at least 2) that doubles before count + inserts would pass half of it; a slot is
 * chosen by a 64-bit mix of all eight words with `salt` (0: drawn from the OS CSPRNG), since users choose their nullifiers.
 * Fees: a 256-bit counter of the `fee` signal of every transaction zkr_ledger_sequence and the replays apply while the book is
 * open (RollUp.sol:139), modulo 2^256 as the contract's uint256.
 *
 * zkr_ledger_book_open: blob NULL = an empty set and zero fees, else a ZKRBOOK1 blob (below); zkr_book_blob_check's refusals are
 * ZKR_ERR_ARG, before the device; a blob that holds one nullifier twice is ZKR_ERR_BAD_KEY.  A second open is ZKR_ERR_ARG.
 * zkr_ledger_book_info: out = distinct keys, nullifiers, nullifier table slots, key-table builds so far (the open counts).
 *
 * zkr_ledger_deposit_calls = deposit(publicKeyX, publicKeyY) payable (RollUp.sol:255-297) for a list of calls, in order.  pubs:
 * n x 64 B, values (msg.value): n x 32 B, standard form.  status[i] is the first of
 *    1  a key element not below r, or a value not below 2^250       2  the key is new and the tree is full
 *    3  the new balance would not stay below 2^250                   0  applied
 * A refused call is a revert: the following calls go on.  A new key gets the index `accounts so far` (RollUp.sol:279) and nonce
 * 0; a later call of the same list with that key adds to the new account.  indices[i] (may be NULL) = balanceTreeLeafIndex of an
 * applied call, 0xFFFFFFFF of a refused one; events (may be NULL): n x 128 B, pubX pubY balance nonce of the Deposit event
 * (:290-296), zeros for a refused call.
 *
 * zkr_ledger_withdraw_calls = withdraw (RollUp.sol:212-253), or withdrawAll (:193-210) for every call when amounts is NULL.
 * publics: n x 96 B, the public signals publicKey[0] publicKey[1] nullifier; amounts: n x 32 B (any 256-bit number);
 * proof_verdicts: NULL or n bytes as zkr_verify_each returns them.  verdicts[i] is the first of
 *    1  an element of the public signals not below r (the verifier's require)
 *    2  the nullifier is used: in the set, or carried by an EARLIER call of this list that was applied (:224)
 *    3  proof_verdicts[i] != 0 (:229)                                4  the key is not registered
 *    5  amount above the balance (:237)                              6  withdrawAll with a zero balance (:205)
 *    0  applied: the balance goes down, the nullifier goes into the set, the Withdraw event (:246-252) is in events / indices
 * A refused call spends nothing: its nullifier stays free for a later call of the same list.
 * Deliberate differences from the contract: verdict 4 -- the contract would read a zero User and, with amount 0, emit an event
 * for leaf 0 under a foreign key; the codes are tried in the order of this table, so withdrawAll's balance check (:205) comes
 * after the others, which changes which refusal is named and never whether a call is applied; and the leaf IS updated, as the
 * operator's pubsub.ts:19-66 does on the event -- the contract itself never updates its tree in withdraw.
 * zkr_ledger_withdraw_calls_device: the signals are words 1..3 of n witnesses in device memory (d_witnesses_std: a host array of
 * device pointers, the convention of zkr_verify_each_device); the kernels run on `stream`.
 *
 * zkr_ledger_lookup_keys: indices[i] = the account that owns key i (isPublicKeyRegistered / getUserData, RollUp.sol:164-191),
 * 0xFFFFFFFF = not registered.  zkr_ledger_nullifiers_used: used[i] = usedNullifiers[nullifier i] (:58, :224).
 * zkr_ledger_fees = getAccuredFees (:299-301); reset != 0 also zeroes the counter, as withdrawAccuredFees does (:303-309), and
 * is ZKR_ERR_ARG while a checkpoint is open.  zkr_ledger_rollback restores the account count, the nullifier count and the fee
 * counter as at the checkpoint.
 *
 * Blob "ZKRBOOK1", 128 + 32 x count bytes, integers little-endian:
 *     0  "ZKRBOOK1"     8  u64 count     16  48 B zero     64  fees (32 B)
 *    96  tag = zkr_mimcsponge_multihash(count, fees mod 2^128, fees div 2^128)      128  the nullifiers in acceptance order
 * The ZKRLEDG1 snapshot does not change; a snapshot and a blob taken together resume a ledger with its book.
 * zkr_book_blob_check (host only): magic, reserved bytes, length, tag, every nullifier below r; *valid = 0 comes with ZKR_OK and
 * a zkr_last_error line naming the first failure; info = count, byte length.  The Node binding does not carry the book. ---- */
typedef struct { uint32_t nullifier_cap_log2; uint32_t reserved; uint64_t salt; } zkr_book_opts; /* NULL or zeros = defaults */
int zkr_ledger_book_open(zkr_ledger *l, const zkr_book_opts *opts, const void *blob, size_t blob_len);
int zkr_ledger_book_info(const zkr_ledger *l, uint64_t out[4]);
int zkr_ledger_deposit_calls(zkr_ledger *l, const uint8_t *pubs, const uint8_t *values, size_t n, uint8_t *status, uint32_t *indices,
                             uint8_t *events);
int zkr_ledger_withdraw_calls(zkr_ledger *l, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts, size_t n,
                              uint8_t *verdicts, uint32_t *indices, uint8_t *events);
int zkr_ledger_withdraw_calls_device(zkr_ledger *l, const void *const *d_witnesses_std, const uint8_t *amounts,
                                     const uint8_t *proof_verdicts, size_t n, uint8_t *verdicts, uint32_t *indices, uint8_t *events,
                                     void *stream);
int zkr_ledger_lookup_keys(zkr_ledger *l, const uint8_t *pubs, size_t n, uint32_t *indices);
int zkr_ledger_nullifiers_used(zkr_ledger *l, const uint8_t *nullifiers, size_t n, uint8_t *used);
int zkr_ledger_fees(const zkr_ledger *l, uint8_t fees[32], int reset);
int zkr_ledger_book_blob(const zkr_ledger *l, void **blob, size_t *len); /* malloc'ed, free with zkr_free */
int zkr_book_blob_check(const void *blob, size_t len, uint64_t info[2], int *valid);
/* Test hooks, host only, as zkr_sequence_plan_host is: the host pass alone over records = n_accounts x 128 B.  resolved: n x 3
 * words per call as the resolve kernel leaves them -- flags (1 pubX below r, 2 pubY below r, 4 nullifier below r, 8 nullifier in
 * the set), the key's account or 0xFFFFFFFF, the call's leader: the lowest list position with the same key (deposits) or the
 * same nullifier (withdrawals).  ZKR_ERR_ARG when `resolved` cannot be true of these records and this list. */
int zkr_book_deposit_plan_host(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *pubs, const uint8_t *values,
                               size_t n, const uint32_t *resolved, uint8_t *status, uint32_t *indices, uint8_t *events);
int zkr_book_withdraw_plan_host(const uint8_t *records, size_t n_accounts, const uint8_t *publics, const uint8_t *amounts,
                                const uint8_t *proof_verdicts, size_t n, const uint32_t *resolved, uint8_t *verdicts,
                                uint32_t *indices, uint8_t *events);

/* ---- the operator's step: a signed queue in, verified proofs out, behind one handle (csrc/zkr_operator.hip).
 * The loop around a proof (operator/src/routes/send.ts:72-135, pubsub.ts:19-66, snarks/common.ts:12-38) is zkr_ledger_sequence ->
 * zkr_rollup_witness_batch_from_device -> zkr_r1cs_check_device -> zkr_prove_batch_device -> zkr_verify_each_device, and it hands
 * DEVICE buffers from call to call.  An operator owns those buffers, so its caller passes host buffers only (what the Node binding
 * can do), and it closes the gap a hand-written loop leaves: the sequencing advances the ledger before anything is proved, so a
 * later failure leaves the ledger ahead of what can be published.  A step runs inside a ledger checkpoint of its own and the
 * ledger moves only when every proof of the step is good.  No kernel of its own: the calls above launch what they launch alone.
 *
 * zkr_operator_new.  The four handles are BORROWED: the caller keeps them alive longer than the operator.  cs NULL: no constraint
 * check; vk NULL: no acceptance check (zkr_verify_each_device takes about 50 ms whatever the batch size, profiles/verify_device.md:
 * a caller that minds passes NULL and checks on the host with zkr_verify_batch).  opts: batch = transactions per proof;
 * max_batches = the most proofs one step may produce (0: 256); flags and reserved 0.  Checked before anything is allocated, each
 * failure ZKR_ERR_ARG with a message naming the mismatch: all handles on one device; zkr_rollup_info(batch, the ledger's depth)
 * gives the key's nVars and nPublic; cs is the key's by zkr_r1cs_matches_key; vk has the key's nPublic.
 * The handle owns, on that device: the circuit inputs and the witnesses of a step (n_batches x (nPublic - 1) x 32 B and n_batches x
 * nVars x 32 B), the array of witness pointers (pinned host memory) and one stream.  They grow to the largest step seen, at most
 * max_batches.  zkr_operator_info: out = batch, depth, nVars, nPublic, max_batches, device bytes held.
 *
 * zkr_operator_step.  txs (n_txs x 8 x 32 B) and status (n_txs bytes) as zkr_ledger_sequence takes and gives them; r32s / s32s as
 * zkr_prove_batch_device: n_txs / batch x 32 B each, proof b takes row b, or both NULL (drawn per proof); proofs_out: room for
 * n_txs / batch proofs of 256 B; publics_out: room for as many rows of nPublic x 32 B -- words 1..nPublic of each witness, one
 * strided copy from the device.  Steps on one operator are serialised by a lock inside it.  In order: open a checkpoint, sequence
 * on the operator's stream, build the witnesses from the device inputs, check them against cs, prove, zkr_verify_each_device
 * against vk, read out, release the checkpoint.
 *   n_txs / batch > max_batches: ZKR_ERR_ARG before the ledger or any buffer is touched.
 *   No whole batch: ZKR_OK, *n_batches = 0, statuses and *consumed as zkr_ledger_sequence gives them, no checkpoint left open.
 *   Any failure after the sequencing: the ledger is rolled back to the step's checkpoint, the checkpoint is released and the
 *   status is returned -- ZKR_ERR_UNSATISFIED for inputs the circuit refuses or a violated constraint (the message names the
 *   batch), the prover's own code for its errors, ZKR_ERR_BAD_KEY "batch b: proof rejected by the verifying key (verdict v)" for a
 *   verdict other than 0.  Records, account count, every byte of the stored tree, applied and batches are then as before the call.
 * Outputs are defined only on ZKR_OK.  The step's checkpoint nests inside the caller's: a later zkr_ledger_rollback to an older
 * checkpoint still undoes a successful step.
 * zkr_operator_stage_times: wall milliseconds of the last step's stages -- sequence, witness, check, prove, verify, read-out (every
 * stage returns synchronised; 0 for a stage that did not run). ---- */
typedef struct zkr_operator zkr_operator;
typedef struct { uint32_t batch, max_batches, flags, reserved; } zkr_operator_opts;
int zkr_operator_new(zkr_ledger *l, zkr_key *key, zkr_r1cs *cs, zkr_vk *vk, const zkr_operator_opts *opts, zkr_operator **out);
void zkr_operator_free(zkr_operator *op);
int zkr_operator_info(const zkr_operator *op, uint64_t out[6]);
int zkr_operator_step(zkr_operator *op, const uint8_t *txs, size_t n_txs, const uint8_t *r32s, const uint8_t *s32s, uint8_t *status, uint8_t *proofs_out,
                      void *publics_out, size_t *n_batches, size_t *consumed);
int zkr_operator_stage_times(const zkr_operator *op, double ms[6]);

/* Integer-ALU microbenchmark: sustained Fq Montgomery multiplications per second on `device` with the multiplier of the
 * hot path (9 x 29-bit limbs, 162 multiply-adds without carry words, csrc/field29.hpp); used for the secondary (VALU)
 * roofline.  _legacy: the 8 x 32-bit multiplier of csrc/field.hpp (136 multiply-adds + 136 carry additions), kept for
 * the boundary formats and the cold kernels. */
/* Limb-level self test of the hot path's Montgomery product forms (csrc/field29.hpp: 9 x 29-bit limbs, radix 2^261) as the
 * device runs them.  records: n x 8 operands x 9 raw limbs (a b c d e f g h; limbs below 2^29, the top limb free);
 * out: n x 9 raw limbs of form 0: a b, 1: a^2, 2: a b + c d, 3: a b + c d + e f + g h (x 2^-261 mod the field's modulus,
 * lazily reduced).  field 0 = Fq, 1 = Fr.  The host build of the same header (libzkr_hostarith.so zkt29_raw_forms) must
 * give the same limbs bit for bit: tests/test_gpu_stages.py. */
int zkr_selftest_f29_forms(int device, int field, int form, const uint32_t *records, size_t n, uint32_t *out);
/* The same one layer up: the group law of the hot path (csrc/curve29.hpp) on raw limbs as the device compiles it, one thread per
 * record.  g2: 0 = G1 over Fq (9 limbs per coordinate), 1 = G2 over Fq2 (18: re, im); the low eight limbs of a value below 2^29,
 * the top limb = value >> 232, values x 2^261, nothing reduced on the way in or out.  op and record (csrc/curve29_raw.hpp):
 * 0 add_mixed29 (X Y ZZ ZZZ, qx qy; flag neg_q), 1 add_affine_affine29 (ax ay, bx by; flags neg_a, neg_b), 2 add_full29 (two
 * XYZZ; the second is read again for the doubling), 3 dbl_xyzz29, 4 dbl_affine29 (x y), 5 dbl_jac29 (X Y Z), 6 pack_xyzz and
 * unpack_xyzz of the result; a record = its coordinates, then two flag words.  out: n x (4 coordinates; op 5: 3; op 6: the 4
 * packed coordinates of 8 / 16 words, then the 4 read back as limbs); inf: n bytes, 1 = the point at infinity.  The host build
 * of the same header (libzkr_hostarith.so zkt29_curve_raw) must give the same limbs: tests/test_gpu_group_law.py. */
int zkr_selftest_curve29(int device, int g2, int op, const uint32_t *records, size_t n, uint32_t *out, uint8_t *inf);
/* And one layer down, off the hot path: the 8 x 32-bit-limb field of csrc/field.hpp (radix 2^256) as the device compiles it -- the
 * product scanning in a 96-bit column accumulator, the fused sums of csrc/field_fused.hpp, the schoolbook Fq2 product and both
 * mul_sub, none of which the host build shares -- on raw limbs, one thread per record.  records: n x 8 operands x 8 words, least
 * significant word first, nothing converted on the way in or out; an operation ignores the operands it does not read.  field 0 =
 * Fq, 1 = Fr.  op (csrc/field_raw_ops.def): 0 mul(a,b), 1 sqr(a), 2 add(a,b), 3 sub(a,b), 4 neg(a), 5 reduce_once(a),
 * 6 mul_sum2(a,b,c,d), 7 mul_sum4(a..h), 8 mul_sub(a,b,c,d), 9 to_mont(a), 10 from_mont(a), 11 inv(a); out: n x 8 words.  Over Fq2
 * (field 0 only; an element = two operands, re then im): 12 mul(x,y), 13 sqr(x), 14 mul_sub(x,y,z,w), 15 inv(x); out: n x 16
 * words.  Every result is canonical, so the host build of the same function (libzkr_hostarith.so zkt_fp_raw) and integer
 * arithmetic must give the same words bit for bit: tests/test_gpu_field_raw.py. */
int zkr_selftest_fp(int device, int field, int op, const uint32_t *records, size_t n, uint32_t *out);
/* The NTT pass kernel (csrc/kernels_ntt.hpp) in every mode its two host drivers launch it in, alone: exactly ONE run_ntt
 * (cross = 0) or ONE run_ntt_cross (cross = 1) of csrc/zkr_prove.hip -- the code objects the proofs launch -- on host-supplied
 * vectors, the raw result back: no bit-reversal copy, no 1/n.  Twiddle tables are built for 2^tlog as zkr_ntt builds them for
 * 2^logn.  Every field is checked before any launch (ZKR_ERR_ARG and a message):
 *   logn 1..22; tlog logn + coset_shift .. 24; dif, inverse, pair, in_place, canon, cross 0 / 1; pre 0 none, 1 coset (position gi
 *   times g^(((bitrev(gi) << coset_shift) | coset_add) << (tlog - logn - coset_shift)), g = w_{2^(tlog+1)}; coset_add below
 *   2^coset_shift, both 0 without it), 2 product with in1 (x y / 2^256); nbat >= 1 vectors end to end (nbat 2^logn <= 2^24);
 *   want_lo / want_n: run_ntt's output range (0, 0 = all; run_ntt itself refuses a range of a DIT transform or one outside it).
 *   cross: klog 1..3 below logn, columns [col_lo, col_lo + col_n) of the 2^klog row blocks of 2^(logn - klog) elements, col_lo and
 *   col_n multiples of the tile width run_ntt_cross picks; in_sub / out_sub 0 or col_lo; pre 0 or 2; tlog >= logn; nbat 1, no pair,
 *   no range, no coset fields; canon as given (cross = 0: run_ntt decides).
 * Vectors are host buffers of 32-byte little-endian standard-form words, all IN and OUT: each is copied to the device (in0, in1
 * and their _b twins through the ingest kernel, as zkr_ntt does; out as it is), and copied back after the run, so a caller sees
 * that an out-of-place transform left its inputs alone and what it left of `out` outside the range or the columns it was asked for.
 * cross = 0: every vector nbat 2^logn words.  cross = 1: the 2^klog row blocks end to end, 2^(logn - klog) words each -- col_n
 * words each for in0 / in1 when in_sub != 0 and for out when out_sub != 0 (a local buffer of this shard's columns) -- and every
 * block in a device allocation of its own.  in1 (in1_b): pre == 2 only; out (out_b): in_place == 0 only -- in place the result
 * comes back in in0 (cross: in_sub == out_sub); the _b vectors: pair == 1 only.  Unused ones may be NULL.
 * Every device vector lies between two guard regions of a fixed pattern, read back after the run: a changed guard is ZKR_ERR_HIP
 * with a message naming the vector (the vectors are still copied back).  tests/test_gpu_ntt_modes.py, tests/ntt_cases.py. */
typedef struct {
  uint32_t logn, tlog, dif, inverse, pre, nbat, pair, in_place, want_lo, want_n, coset_shift, coset_add;
  uint32_t cross, klog, col_lo, col_n, in_sub, out_sub, canon, reserved;
} zkr_ntt_selftest_desc;
int zkr_selftest_ntt(int device, const zkr_ntt_selftest_desc *desc, void *in0, void *in1, void *out, void *in0_b, void *in1_b, void *out_b);
int zkr_bench_fq_mul(int device, double *gmuls_per_s);
int zkr_bench_fq_mul_legacy(int device, double *gmuls_per_s);

#ifdef __cplusplus
}
#endif
#endif /* ZKR_H */
