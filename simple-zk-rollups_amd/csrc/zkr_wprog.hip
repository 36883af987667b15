// zkr_wprog.hip -- witness programs on the device: batch witnesses for ANY circuit (zkr_wprog_*, include/zkr.h).
//
// rollup_witness.hpp and wallet_program.hpp are device programs written by hand for this build's two circuits.  A witness program
// (wprog_bin) is data: a straight-line list of field operations over a store of wires, produced by a front end (python/zkr_hip/
// circuit.py is one) together with the circuit's r1cs_bin.  wprog.hpp parses and validates it and holds the interpreter's one
// step, wp_exec; this unit runs it:
//
//   wprog_run_kernel     one lane per instance.  Every lane executes the same instruction: the fetch is indexed by the loop counter
//                        alone, so it is a wave-uniform (scalar) load and the opcode switch does not diverge.  The wire store is
//                        device memory laid out [wire][instance]: the 64 lanes of a wavefront read and write 64 consecutive 32-byte
//                        elements.  Values stay in Montgomery form.  No LDS, no barrier, no private memory.
//   wprog_layout_kernel  gathers map[s] for every witness signal, leaves Montgomery form and writes each instance's witness
//                        contiguously (nVars x 32 B, what zkr_prove_batch_device and zkr_r1cs_check_device take); an instance that
//                        failed gets zeros.
//
// A batch goes through the store in pieces of `piece` instances (the handle's one workspace: n_wires x piece x 32 B).
#include <string.h>
#include "wprog.hpp"
#include "zkr_internal.hpp"

namespace zkr {
const Fr *mimc_round_constants();  // rollup.cpp: the 220 round constants, Montgomery

constexpr int WP_RUN_THREADS = 64;      // one wavefront to a block: a piece spreads over as many CUs as it has wavefronts
constexpr int WP_LAYOUT_THREADS = 256;
constexpr uint32_t WP_LAYOUT_MAX_BLOCKS = 1u << 20;
constexpr size_t WP_STORE_BUDGET = (size_t)1 << 30;  // the default piece: the most instances whose store fits this,
constexpr uint32_t WP_PIECE_MIN = 64, WP_PIECE_DEFAULT_MAX = 16384, WP_PIECE_MAX = 1u << 20;  // a multiple of 64 within these

struct WpRunArgs {
  const WpInstr *__restrict__ ins;
  const Fr *__restrict__ consts;
  const Fr *__restrict__ inputs;  // cnt x n_inputs, standard form
  Fr *store;                      // n_wires x piece
  uint32_t *rep;                  // cnt x 2: code, statement
  uint32_t n_instr, n_inputs, piece, cnt;
};

static __global__ __launch_bounds__(WP_RUN_THREADS) void wprog_run_kernel(WpRunArgs a) {
  const uint32_t j = blockIdx.x * WP_RUN_THREADS + threadIdx.x;
  if (j >= a.cnt) return;
  WpLane L;
  L.store = a.store + j;
  L.stride = a.piece;
  L.consts = a.consts;
  if (wp_begin(L, a.inputs + (size_t)j * a.n_inputs, a.n_inputs))
    for (uint32_t i = 0; i < a.n_instr; i++) wp_exec(L, a.ins[i]);
  a.rep[2 * j] = L.code;
  a.rep[2 * j + 1] = L.stmt;
}

struct WpLayoutArgs {
  const uint32_t *__restrict__ map;
  const Fr *__restrict__ store;
  const uint32_t *__restrict__ rep;
  Fr *out;  // cnt x n_vars, standard form
  uint32_t n_vars, piece, cnt;
};

// element e = s * cnt + j: consecutive lanes read consecutive instances of one wire
static __global__ __launch_bounds__(WP_LAYOUT_THREADS) void wprog_layout_kernel(WpLayoutArgs a) {
  const size_t total = (size_t)a.n_vars * a.cnt;
  for (size_t e = (size_t)blockIdx.x * WP_LAYOUT_THREADS + threadIdx.x; e < total; e += (size_t)gridDim.x * WP_LAYOUT_THREADS) {
    const uint32_t s = (uint32_t)(e / a.cnt), j = (uint32_t)(e % a.cnt);
    Fr v = Fr::zero();
    if (a.rep[2 * j] == WP_OK) v = from_mont(wp_load(a.store + (size_t)a.map[s] * a.piece + j));
    wp_store(a.out + (size_t)j * a.n_vars + s, v);
  }
}

}  // namespace zkr

using namespace zkr;

struct zkr_wprog {
  int device = 0;
  WpProgram p;  // the host copy: counts (the vectors are dropped after the upload)
  uint32_t piece = 0;
  size_t workspace_bytes = 0;
  DevBuf d_ins, d_consts, d_map, d_store, d_rep;
  Pinned<uint32_t> h_rep;
  OwnStream stream;
  ScopedEvent ev;             // "the caller's stream has come this far"
  ScopedEvent t0, t1, t2;     // around the two kernels of a piece
  double ms_run = 0, ms_layout = 0;  // of the last call
};

static int wp_upload(DevBuf &d, const void *src, size_t bytes) {
  if (int rc = d.alloc(bytes)) return rc;
  if (bytes) ZKR_HIP_CHECK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
  return 0;
}

static int wprog_upload(zkr_wprog *w) {
  ZKR_HIP_CHECK(hipSetDevice(w->device));
  const WpProgram &p = w->p;
  int rc;
  if ((rc = wp_upload(w->d_ins, p.ins.data(), p.ins.size() * sizeof(WpInstr))) || (rc = wp_upload(w->d_consts, p.consts.data(), p.consts.size() * sizeof(Fr))) ||
      (rc = wp_upload(w->d_map, p.map.data(), p.map.size() * 4)))
    return rc;
  const size_t store = (size_t)p.n_wires * w->piece * sizeof(Fr), rep = (size_t)w->piece * 8;
  if ((rc = w->d_store.alloc(store)) || (rc = w->d_rep.alloc(rep)) || (rc = w->h_rep.alloc((size_t)w->piece * 2)) || (rc = w->stream.create()) ||
      (rc = w->ev.create(hipEventDisableTiming)) || (rc = w->t0.create()) || (rc = w->t1.create()) || (rc = w->t2.create()))
    return rc;
  w->workspace_bytes = store + rep;
  return 0;
}

static const char *wp_code_text(uint32_t code) { return code == WP_INPUT_RANGE ? "an input is not below r" : "an assertion failed"; }

extern "C" {

int zkr_wprog_load_opts(const void *wprog_bin, size_t len, int device, const zkr_wprog_opts *opts, zkr_wprog **out) {
  if (!wprog_bin || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  *out = nullptr;
  zkr_wprog *w = new zkr_wprog();
  std::string err;
  if (!wprog_parse(wprog_bin, len, w->p, err)) {  // before any device call: a malformed program is refused without a GPU too
    delete w;
    set_error("%s", err.c_str());
    return ZKR_ERR_ARG;
  }
  uint32_t piece = opts ? opts->piece : 0;
  if (opts && opts->reserved) { delete w; set_error("zkr_wprog_opts: reserved is %u, not 0", opts->reserved); return ZKR_ERR_ARG; }
  if (piece == 0) {
    const size_t fit = WP_STORE_BUDGET / ((size_t)w->p.n_wires * sizeof(Fr)) / 64 * 64;
    piece = fit < WP_PIECE_MIN ? WP_PIECE_MIN : fit > WP_PIECE_DEFAULT_MAX ? WP_PIECE_DEFAULT_MAX : (uint32_t)fit;
  }
  if (piece > WP_PIECE_MAX) { delete w; set_error("zkr_wprog_opts: piece = %u is above %u", piece, WP_PIECE_MAX); return ZKR_ERR_ARG; }
  if (int rc = need_device(device, "a witness program (zkr_wprog_run_host runs one instance on the host)")) { delete w; return rc; }
  w->device = device;
  w->piece = piece;
  if (int rc = wprog_upload(w)) { delete w; return rc; }
  w->p.consts = std::vector<Fr>();
  w->p.ins = std::vector<WpInstr>();
  w->p.map = std::vector<uint32_t>();
  *out = w;
  return ZKR_OK;
}

int zkr_wprog_load(const void *wprog_bin, size_t len, int device, zkr_wprog **out) { return zkr_wprog_load_opts(wprog_bin, len, device, nullptr, out); }

void zkr_wprog_free(zkr_wprog *w) {
  if (!w) return;
  (void)hipSetDevice(w->device);
  delete w;
}

int zkr_wprog_info(const zkr_wprog *w, uint64_t out[8]) {
  if (!w || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  out[0] = w->p.n_inputs; out[1] = w->p.n_wires; out[2] = w->p.n_instr; out[3] = w->p.n_vars; out[4] = w->p.n_public;
  out[5] = w->workspace_bytes; out[6] = w->piece; out[7] = w->p.n_statements;
  return ZKR_OK;
}

int zkr_wprog_stage_times(const zkr_wprog *w, double out_ms[2]) {
  if (!w || !out_ms) { set_error("null argument"); return ZKR_ERR_ARG; }
  out_ms[0] = w->ms_run;
  out_ms[1] = w->ms_layout;
  return ZKR_OK;
}

int zkr_wprog_witness_batch_device(zkr_wprog *w, const void *d_inputs_std, size_t n, void *d_witnesses, uint32_t *reports, void *stream) {
  if (!w || (n && (!d_witnesses || (!d_inputs_std && w->p.n_inputs)))) { set_error("null argument"); return ZKR_ERR_ARG; }
  if (((uintptr_t)d_inputs_std | (uintptr_t)d_witnesses) & 15) { set_error("device buffers must be 16-byte aligned"); return ZKR_ERR_ARG; }
  w->ms_run = w->ms_layout = 0;
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(w->device));
  const hipStream_t st = w->stream;
  ZKR_HIP_CHECK(hipEventRecord(w->ev, (hipStream_t)stream));  // the inputs are in place once the caller's stream has come this far
  ZKR_HIP_CHECK(hipStreamWaitEvent(st, w->ev, 0));
  const WpProgram &p = w->p;
  size_t bad = n;  // the first failing instance, for the message
  uint32_t bad_code = 0, bad_stmt = 0;
  for (size_t j0 = 0; j0 < n; j0 += w->piece) {
    const uint32_t cnt = (uint32_t)(n - j0 < w->piece ? n - j0 : w->piece);
    WpRunArgs ra;
    ra.ins = w->d_ins.as<WpInstr>();
    ra.consts = w->d_consts.as<Fr>();
    ra.inputs = static_cast<const Fr *>(d_inputs_std) + j0 * p.n_inputs;
    ra.store = w->d_store.as<Fr>();
    ra.rep = w->d_rep.as<uint32_t>();
    ra.n_instr = p.n_instr; ra.n_inputs = p.n_inputs; ra.piece = w->piece; ra.cnt = cnt;
    WpLayoutArgs la;
    la.map = w->d_map.as<uint32_t>();
    la.store = ra.store;
    la.rep = ra.rep;
    la.out = static_cast<Fr *>(d_witnesses) + j0 * p.n_vars;
    la.n_vars = p.n_vars; la.piece = w->piece; la.cnt = cnt;
    const size_t elems = (size_t)p.n_vars * cnt, want = (elems + WP_LAYOUT_THREADS - 1) / WP_LAYOUT_THREADS;
    const unsigned lblocks = (unsigned)(want > WP_LAYOUT_MAX_BLOCKS ? WP_LAYOUT_MAX_BLOCKS : want);
    ZKR_HIP_CHECK(hipEventRecord(w->t0, st));
    wprog_run_kernel<<<(cnt + WP_RUN_THREADS - 1) / WP_RUN_THREADS, WP_RUN_THREADS, 0, st>>>(ra);
    ZKR_HIP_CHECK(hipEventRecord(w->t1, st));
    wprog_layout_kernel<<<lblocks, WP_LAYOUT_THREADS, 0, st>>>(la);
    ZKR_HIP_CHECK(hipEventRecord(w->t2, st));
    ZKR_HIP_CHECK(hipGetLastError());
    ZKR_HIP_CHECK(hipMemcpyAsync(w->h_rep, w->d_rep.p, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
    ZKR_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0;
    ZKR_HIP_CHECK(hipEventElapsedTime(&ms, w->t0, w->t1));
    w->ms_run += ms;
    ZKR_HIP_CHECK(hipEventElapsedTime(&ms, w->t1, w->t2));
    w->ms_layout += ms;
    if (reports) memcpy(reports + 2 * j0, w->h_rep, (size_t)cnt * 8);
    for (uint32_t j = 0; j < cnt && bad == n; j++)
      if (w->h_rep[2 * j]) { bad = j0 + j; bad_code = w->h_rep[2 * j]; bad_stmt = w->h_rep[2 * j + 1]; }
  }
  if (bad < n) {
    if (bad_code == WP_INPUT_RANGE) set_error("instance %zu: input %u is not below r", bad, bad_stmt);
    else set_error("instance %zu violates statement %u", bad, bad_stmt);
    return ZKR_ERR_UNSATISFIED;
  }
  return ZKR_OK;
}

int zkr_wprog_witness_batch(zkr_wprog *w, const uint8_t *inputs_std, size_t n, void *d_witnesses, uint32_t *reports) {
  if (!w || (n && (!d_witnesses || (!inputs_std && w->p.n_inputs)))) { set_error("null argument"); return ZKR_ERR_ARG; }
  const size_t ni = w->p.n_inputs;
  for (size_t e = 0; e < n * ni; e++) {  // before the device is looked at
    uint32_t x[8];
    memcpy(x, inputs_std + 32 * e, 32);
    if (!words_below(x, FrParams::P)) { set_error("instance %zu: input %zu (element %zu) is not below r", e / ni, e % ni, e); return ZKR_ERR_ARG; }
  }
  if (n == 0) return ZKR_OK;
  ZKR_HIP_CHECK(hipSetDevice(w->device));
  DevBuf d_in;
  if (int rc = wp_upload(d_in, inputs_std, n * ni * 32)) return rc;
  return zkr_wprog_witness_batch_device(w, d_in.p, n, d_witnesses, reports, nullptr);
}

int zkr_wprog_run_host(const void *wprog_bin, size_t len, const uint8_t *inputs_std, uint8_t *witness_out, uint8_t *wires_out, uint32_t *code, uint32_t *stmt) {
  if (!wprog_bin || !witness_out || !code || !stmt) { set_error("null argument"); return ZKR_ERR_ARG; }
  WpProgram p;
  std::string err;
  if (!wprog_parse(wprog_bin, len, p, err)) { set_error("%s", err.c_str()); return ZKR_ERR_ARG; }
  if (!inputs_std && p.n_inputs) { set_error("null argument"); return ZKR_ERR_ARG; }
  wprog_run_host(p, inputs_std, witness_out, wires_out, code, stmt);
  if (*code) set_error("%s (statement %u)", wp_code_text(*code), *stmt);
  return ZKR_OK;
}

int zkr_wprog_shape(const void *wprog_bin, size_t len, uint64_t out[8]) {
  if (!wprog_bin || !out) { set_error("null argument"); return ZKR_ERR_ARG; }
  WpProgram p;
  std::string err;
  if (!wprog_parse(wprog_bin, len, p, err)) { set_error("%s", err.c_str()); return ZKR_ERR_ARG; }
  out[0] = p.n_inputs; out[1] = p.n_wires; out[2] = p.n_instr; out[3] = p.n_vars; out[4] = p.n_public; out[5] = 0; out[6] = 0; out[7] = p.n_statements;
  return ZKR_OK;
}

int zkr_mimcsponge_round_constants(uint8_t *out) {
  if (!out) { set_error("null argument"); return ZKR_ERR_ARG; }
  const Fr *c = mimc_round_constants();
  for (int i = 0; i < 220; i++) {
    const Fr s = from_mont(c[i]);
    memcpy(out + 32 * i, s.v, 32);
  }
  return ZKR_OK;
}

}  // extern "C"
