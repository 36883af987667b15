// Types for the Node.js host of the MI355X Groth16 prover (mirrors the websnark / snarkjs surfaces the
// reference uses: operator/src/snarks/common.ts:4-5,23,29).
export interface Groth16Proof {
  pi_a: [string, string, string];
  pi_b: [[string, string], [string, string], [string, string]];
  pi_c: [string, string, string];
  protocol?: "groth";
}
/** devices (groth16GenProof): ONE proof over these GPUs -- the key is cut into devices.length shards (cached), the proof is the same bytes. */
export interface ProveOptions { r?: bigint | string; s?: bigint | string; device?: number; devices?: number[]; }
/** devices: HIP ordinals of the GPUs a batch is sharded over (a device may be listed twice: two proof pipelines on it). */
export interface BatchOptions { devices?: number[]; blinding?: ProveOptions[]; }
/** piecePoints: output points per table converted and copied at a time (default 2^20). */
export interface KeyExportOptions { piecePoints?: number; }
/** A device key as a native handle (what keyEvalTables, keyHForm and keyReplication take). */
export type KeyHandle = unknown;
/** snarkjs 0.1.20 proving key, as the reference's `*_pk.json` holds it and binarifyProvingKey reads it: decimal strings. */
export interface ProvingKeyJson {
  protocol: "groth"; nVars: number; nPublic: number; domainBits: number; domainSize: number;
  polsA: Array<{ [constraint: string]: string }>; polsB: Array<{ [constraint: string]: string }>;
  A: string[][]; B1: string[][]; B2: string[][][]; C: Array<string[] | null>; hExps: string[][];
  vk_alfa_1: string[]; vk_beta_1: string[]; vk_delta_1: string[]; vk_beta_2: string[][]; vk_delta_2: string[][];
}
export interface Bn128 {
  /** websnark-compatible: ArrayBuffers produced by binarifyWitness / binarifyProvingKey. */
  groth16GenProof(witnessBin: ArrayBuffer | Uint8Array, provingKeyBin: ArrayBuffer | Uint8Array, opts?: ProveOptions): Promise<Groth16Proof>;
  /** Independent proofs on one key in one native call: pipelined two deep, proofs of small circuits fused into shared launches. */
  /** opts: per-proof blinding (array), or { devices, blinding }: the batch is sharded over the listed GPUs of this node
   *  (proof i on devices[i % devices.length]; the key is parsed once and copied device to device to the others). */
  groth16GenProofBatch(witnessBins: Array<ArrayBuffer | Uint8Array>, provingKeyBin: ArrayBuffer | Uint8Array, opts?: ProveOptions[] | BatchOptions): Promise<Groth16Proof[]>;
  /** The same with the key currently held on the device. */
  proveBatch(witnessBins: Array<ArrayBuffer | Uint8Array>, opts?: ProveOptions[] | BatchOptions): Promise<Groth16Proof[]>;
  /** Groth16 setup of circom's circuit JSON on the GPU (snarkjs setup --protocol groth); returns the verifying key JSON. */
  setup(circuitDef: any, opts?: { toxic?: Array<bigint | string> }): any;
  /** The same for a constraint system in the r1cs_bin layout (RollupCircuit.r1cs()). */
  setupR1cs(r1csBin: Uint8Array, opts?: { toxic?: Array<bigint | string> }): any;
  /** A further party's contribution to the held key's delta (zkr_key_contribute): the object's key becomes the contributed one;
   *  returns the 352-byte record.  opts.d: the secret (1 < d < r) for reproducible tests; by default drawn inside the library. */
  contribute(opts?: { d?: bigint | string }): { record: Uint8Array };
  /** Evaluation-form side tables for the held key from its own points and the circuit's C side (zkr_key_eval_tables): true when
   *  its proofs run four transforms instead of six from now on (the fused groups of proveBatch included).  contribute, saveKey / loadKeyFile and replicas carry no tables. */
  evalTables(r1csBin: Uint8Array): boolean;
  saveKey(path: string): void;
  /** The held key as the provingKeyBin binarifyProvingKey writes (zkr_key_export_websnark), whatever it came from -- setupR1cs,
   *  loadKeyFile, contribute(): what an unchanged groth16GenProof(witnessBin, provingKeyBin) takes. */
  exportKey(opts?: KeyExportOptions): ArrayBuffer;
  /** The same key as the snarkjs JSON: binarifyProvingKey(bn.exportKeyJson()) equals bn.exportKey(). */
  exportKeyJson(): ProvingKeyJson;
  loadKeyFile(path: string): void;
  /** What the held key's arena contains (zkr_key_check): every index the kernels follow stays inside its section; with
   *  { deep: true } also the values (points on their curves at every window level, twiddles, coefficients, shared rank maps,
   *  header constants).  Returns the clean report (all zero); throws the library's message naming the first faulty section. */
  checkKey(opts?: { deep?: boolean }): { bad: number; section: number; part: number; first: number };
  /** Proof with the key currently held on the device. */
  prove(witnessBin: ArrayBuffer | Uint8Array, opts?: ProveOptions): Promise<Groth16Proof>;
  keyInfo(): { nVars: number; nPublic: number; domainSize: number; nnzA: number; nnzB: number } | null;
  terminate(): void;
}
export function buildBn128(device?: number): Promise<Bn128>;
export function genProof(provingKey: any, witness: Array<bigint | string>, opts?: ProveOptions): Promise<{ proof: Groth16Proof; publicSignals: string[] }>;
export function binarifyWitness(witness: Array<bigint | string>): ArrayBuffer;
export function binarifyProvingKey(provingKey: any): ArrayBuffer;
export function solidityProof(proof: Groth16Proof, publicSignals: Array<bigint | string>): { a: string[]; b: string[][]; c: string[]; inputs: string[] };
/** snarkjs groth.isValid(vk, proof, publicSignals) on the native host verifier (no GPU needed). */
export function isValid(verifyingKey: any, proof: Groth16Proof, publicSignals: Array<bigint | string>): boolean;
/** The record of a delta contribution by itself: points on their curves, the Schnorr proof, the pairing check (host only). */
export function contributionCheck(record: Uint8Array): boolean;
/** vkBin with vk_delta_2 replaced by the record's delta2_after; throws for a bad record or one that does not continue this key. */
export function vkContribute(vkBin: Uint8Array, record: Uint8Array): Uint8Array;
/** All proofs of a batch under one key with one merged pairing product (random linear combination). */
/** exportKey for a key handle. */
export function keyToWebsnark(key: KeyHandle, opts?: KeyExportOptions): ArrayBuffer;
/** The JSON key from the standard-form export (zkr_key_export_websnark with ZKR_EXPORT_STANDARD), which exportKeyJson reads. */
export function jsonKeyFromStandard(standardBytes: Uint8Array): ProvingKeyJson;
export function isValidBatch(verifyingKey: any, proofs: Groth16Proof[], publicSignalsList: Array<Array<bigint | string>>): boolean;
export function binarifyVerifyingKey(verifyingKey: any): Uint8Array;
export function binarifyR1cs(circuitDef: any): Uint8Array;
export function verifyingKeyFromBytes(vkBin: Uint8Array): any;
export function proofFromBytes(proofBytes: Uint8Array): Groth16Proof;
export function deviceCount(): number;
export function version(): string;

// ---- the rollup circuit without circom / snarkjs (operator/src/utils/crypto.ts, prover/circuits/batchprocesstx.circom)
export interface Signature { R8: [bigint, bigint]; S: bigint; }
export function multiHash(values: Array<bigint | string | number>): bigint;
export function hashLeftRight(left: bigint, right: bigint): bigint;
/** multiHash of every row on the GPU (one thread per hash). */
export function multiHashBatch(rows: Array<Array<bigint | string | number>>, device?: number): bigint[];
/** The reference's balance tree over the leaves (padded to 2^depth), hashed on the GPU. */
export function buildBalanceTree(depth: number, leaves: Array<bigint | string>, zeroValue?: bigint, device?: number): { depth: number; levels: bigint[][]; root: bigint; path(i: number): bigint[] };
export function genPublicKey(privKey: bigint): [bigint, bigint];
export function formatPrivKeyForBabyJub(privKey: bigint): bigint;
export function sign(privKey: bigint, msg: Array<bigint | string | number>): Signature;
export function verify(msg: Array<bigint | string | number>, sig: Signature, pubKey: [bigint, bigint]): boolean;
/** types/primitives.ts:40.  Each element is the integer msg[i] + mimc7.hash(key, iv + i), below 2r. */
export interface EncryptedMessage { iv: bigint; msg: bigint[]; }
/** ecdh (crypto.ts:86-93).  Throws for a public key that is not on the curve. */
export function ecdh(privKey: bigint, pubKey: [bigint, bigint]): bigint;
export function encrypt(msg: Array<bigint | string | number>, key: bigint): EncryptedMessage;
export function decrypt(encryptedMsg: EncryptedMessage, key: bigint): bigint[];
export function ecdhEncrypt(msg: Array<bigint | string | number>, privKey: bigint, pubKey: [bigint, bigint]): EncryptedMessage;
export function ecdhDecrypt(encryptedMsg: EncryptedMessage, privKey: bigint, pubKey: [bigint, bigint]): bigint[];
/** BatchProcessTx(batch, depth) (tx.circom = (2, 6)) as constraint system + witness builder. */
export class RollupCircuit {
  constructor(batch?: number, depth?: number);
  readonly batch: number; readonly depth: number; readonly nVars: number; readonly nPublic: number; readonly nConstraints: number;
  r1cs(): Uint8Array;
  /** circuitInputs as the reference builds them (one array per input signal over the batch); throws where Circuit.calculateWitness would. */
  calculateWitness(circuitInputs: { [signal: string]: any } | Array<bigint | string>): ArrayBuffer;
  publicSignals(witnessBin: ArrayBuffer): bigint[];
}
/** Withdraw() (withdraw.circom): public signals publicKey[0], publicKey[1], nullifier. */
export class WithdrawCircuit {
  readonly nPublic: number;
  r1cs(): Uint8Array;
  calculateWitness(circuitInputs: { privateKey: bigint | string; nullifier: bigint | string }): ArrayBuffer;
  publicSignals(witnessBin: ArrayBuffer): bigint[];
}

// ---- the operator's ledger and step on the GPU (send.ts:72-135, pubsub.ts:19-66, snarks/common.ts:12-38), host buffers only
type Num = bigint | string | number;
/** The txData row of one signed transaction: from to amount fee nonce R8x R8y S, 256 bytes. */
export function txRow(from: Num, to: Num, amount: Num, fee: Num, nonce: Num, sig: Signature): Uint8Array;
export type DepositRow = [number, [Num, Num], Num, Num?];
/** Account records and the whole balance tree on the device. */
export class Ledger {
  constructor(depth: number, device?: number);
  readonly depth: number; readonly device: number;
  deposit(index: number, pub: [Num, Num], balance: Num, nonce?: Num): void;
  deposit(rows: DepositRow[]): void;
  root(): bigint;
  account(index: number): { record: bigint[]; path: bigint[] };
  info(): { depth: number; accounts: number; applied: number; batches: number };
  /** The ZKRLEDG1 blob of the current state; restore checks it on the host and refuses records that do not rebuild to its root. */
  snapshot(): Uint8Array;
  static restore(blob: Uint8Array, device?: number): Ledger;
  save(path: string): void;
  static load(path: string, device?: number): Ledger;
  /** Checkpoints nest; rollback(id) puts records, tree and counters back as they stood at checkpoint() and leaves id open. */
  checkpoint(): number;
  rollback(id: number): void;
  release(id: number): void;
  journalInfo(): { checkpoints: number; nodes: number };
  /** Throws while a live Operator holds the ledger. */
  close(): void;
}
export interface OperatorOptions {
  ledger: Ledger;
  /** A Bn128 that holds a key (setupR1cs, loadKeyFile, or a key the cache holds); terminate() throws while the operator lives. */
  bn: Bn128;
  /** The circuit's constraint system (RollupCircuit.r1cs()): every witness is checked against it before proving. */
  r1csBin?: Uint8Array;
  /** vk_bin bytes or the verifying key JSON: every proof is checked on the GPU before the step succeeds. */
  vkBin?: Uint8Array | any;
  batch?: number;
  maxBatches?: number;
}
export interface OperatorBatch { proof: Groth16Proof; publicSignals: string[]; solidityProof: { a: string[]; b: string[][]; c: string[]; inputs: string[] }; }
/** One operator step behind one handle: a signed queue in; statuses, proofs and public signals out; the ledger moves only when every proof is good. */
export class Operator {
  constructor(opts: OperatorOptions);
  readonly batch: number; readonly nPublic: number;
  /** Steps issued on one operator run in issue order; a library error rejects with its message and leaves the ledger as it was. */
  step(queue: Uint8Array[] | Uint8Array, opts?: { rs?: Num[]; ss?: Num[] }): Promise<{ status: number[]; consumed: number; batches: OperatorBatch[] }>;
  info(): { batch: number; depth: number; nVars: number; nPublic: number; maxBatches: number; deviceBytes: number };
  stageTimes(): { sequence: number; witness: number; check: number; prove: number; verify: number; readOut: number };
  close(): void;
}

// ---- process-level key cache (the reference builds a new Bn128 per proof: common.ts:23) and verifier constants
/** Device keys loaded / found in the cache by groth16GenProof so far in this process. */
export function keyCacheStats(): { loads: number; hits: number; replications: number; shardings?: number; entries: number; handles: number; shardedLastForm: ShardedForm };
/** Which form the last sharded proof (groth16GenProof with opts.devices) took and why: calcH split over the shards, or computed by every shard for itself;
 *  hForm / hReason: H in evaluation form (every shard was cut with side tables: the cached key had them) or in coefficient form. */
export interface ShardedForm { form: "none" | "split" | "replicated"; reason: string; hForm: "none" | "coefficients" | "evaluation"; hReason: string }
export function shardedLastForm(): ShardedForm;
/** How a native key handle came to its device: loaded there ("none") or copied device to device (zkr_key_replicate) in the full or the compact form. */
/** zkr_key_eval_tables for a key handle: true when the key proves through the evaluation form from now on. */
export function keyEvalTables(key: unknown, r1csBin: Uint8Array): boolean;
/** zkr_key_h_form for a key handle (a whole key or a shard): whether it has the side tables, and the witnesses proved again so far. */
export function keyHForm(key: unknown): { form: "coefficients" | "evaluation"; retries: number };
export function keyReplication(key: unknown): { mode: "none" | "full" | "base"; peerDirect: boolean };
export function keyFingerprint(provingKeyBin: ArrayBuffer | Uint8Array, full?: boolean): string;
export function clearKeyCache(): void;
/** vk_bin -> the constants of the generated verifier's verifyingKey() in the contract's encoding (G2 as [im, re]). */
export function solidityVerifyingKey(vkBin: Uint8Array): { alfa1: string[]; beta2: string[][]; gamma2: string[][]; delta2: string[][]; IC: string[][] };
/** The Solidity statements of verifyingKey() for those constants (what `snarkjs generateverifier` emits). */
export function solidityVerifyingKeySource(vkBin: Uint8Array, indent?: string): string;
