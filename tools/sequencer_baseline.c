/* sequencer_baseline.c -- what the sequencer replaces, as one host core does it: per transaction one zkr_eddsa_verify and the
 * hashes of two tree updates (a leaf hash of four elements and `depth` hashes of two, twice), through the library's host
 * functions only.  Built by tools/sequencer_time.py into tools/bin/libsequencer_baseline.so; returns wall seconds.
 *   cc -O2 -shared -fPIC tools/sequencer_baseline.c -o tools/bin/libsequencer_baseline.so -Lsimple-zk-rollups_amd/csrc -lzkr_hip */
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <time.h>
#include "../include/zkr.h"

double sequencer_baseline(const uint8_t *txs, const uint8_t *pubs, const uint8_t *records, size_t n, unsigned depth, size_t *n_valid, uint8_t sink[32]) {
  struct timespec t0, t1;
  uint8_t node[64], leaf[32];
  size_t valid = 0;
  memset(node, 0, sizeof node);
  clock_gettime(CLOCK_MONOTONIC, &t0);
  for (size_t t = 0; t < n; t++) {
    int ok = 0;
    zkr_eddsa_verify(txs + t * 256, 5, txs + t * 256 + 160, pubs + t * 64, &ok);
    valid += ok != 0;
    for (int side = 0; side < 2; side++) { /* the sender's leaf, then the recipient's */
      zkr_mimcsponge_multihash(records + (t * 2 + side) * 128, 4, leaf);
      memcpy(node, leaf, 32);
      for (unsigned l = 0; l < depth; l++) { /* hashLeftRight up the path; the sibling is whatever the last step left */
        zkr_mimcsponge_multihash(node, 2, leaf);
        memcpy(node + 32, node, 32);
        memcpy(node, leaf, 32);
      }
    }
  }
  clock_gettime(CLOCK_MONOTONIC, &t1);
  memcpy(sink, node, 32);
  *n_valid = valid;
  return (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
}
