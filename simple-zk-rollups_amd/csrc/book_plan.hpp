// book_plan.hpp -- the HOST pass of the ledger's book (zkr_ledger_deposit_calls / zkr_ledger_withdraw_calls): the
// contract's deposit (RollUp.sol:255-297) and withdraw / withdrawAll (RollUp.sol:193-253) applied to a list of calls in order,
// from what book_resolve_kernel found for every call -- its account, whether its nullifier is spent, its leader in the list --
// and the ledger's records.  The balance arithmetic is sequential and a duplicate depends on what was accepted before it, so
// this part stays on the host, as sequencer_plan.cpp does.  And the ZKRBOOK1 blob: header, tag and parser.  Plain C++ (no HIP):
// zkr_book.hip runs it between its kernels, zkr_book_*_plan_host and zkr_book_blob_check expose it to the CPU suite, and
// book_selfcheck.cpp drives it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "sequencer_plan.hpp"

namespace zkr {

enum : uint32_t { BOOK_NONE = 0xFFFFFFFFu };
// flags of a resolved call entry
enum : uint32_t { BOOK_X_BELOW_R = 1, BOOK_Y_BELOW_R = 2, BOOK_NULL_BELOW_R = 4, BOOK_NULL_USED = 8 };
struct BookResolve {  // what book_resolve_kernel writes per call entry, three words
  uint32_t flags;     // BOOK_* above
  uint32_t account;   // the index the key table holds for the entry's key, or BOOK_NONE
  uint32_t leader;    // the lowest list position with the same key (deposits) / the same nullifier (withdrawals); <= the entry's own
};

enum : uint8_t { DEP_OK = 0, DEP_RANGE = 1, DEP_FULL = 2, DEP_BALANCE = 3 };
enum : uint8_t { WD_OK = 0, WD_RANGE = 1, WD_USED = 2, WD_PROOF = 3, WD_NO_KEY = 4, WD_AMOUNT = 5, WD_ZERO = 6 };

struct BookPlan {
  std::vector<uint8_t> status;     // n: the status / verdict of every call
  std::vector<uint32_t> index;     // n: the account of an applied call, BOOK_NONE of a refused one
  std::vector<uint8_t> events;     // n x 128: pubX pubY balance nonce as the event carries them; zeros for a refused call
  std::vector<uint32_t> upd_idx;   // the update list: one entry per applied call, in list order
  std::vector<uint8_t> upd_rec;    // ... x 128
  std::vector<uint32_t> accepted;  // withdrawals: the list positions whose nullifiers go into the set, in order
  size_t accounts_after = 0;
};

// pubs: n x 64, values: n x 32.  0, or -1 with *why set when `res` cannot have come from these records (an account out of range or
// under another key, a leader behind its entry): nothing the device returned is followed unchecked.
int deposit_plan(unsigned depth, const uint8_t *records, size_t n_accounts, const uint8_t *pubs, const uint8_t *values, size_t n,
                 const BookResolve *res, BookPlan &out, const char **why);
// publics: n x 96 (pubX pubY nullifier), amounts: n x 32 or NULL (every call a withdrawAll), proof_verdicts: n bytes or NULL.
int withdraw_plan(const uint8_t *records, size_t n_accounts, const uint8_t *publics, const uint8_t *amounts, const uint8_t *proof_verdicts,
                  size_t n, const BookResolve *res, BookPlan &out, const char **why);

// ---- the ZKRBOOK1 blob (include/zkr.h)
enum : size_t { BOOK_HEADER_BYTES = 128 };
struct BookHeader {
  uint64_t count = 0;
  uint8_t fees[32] = {0};
};
int book_header_write(const BookHeader &h, uint8_t out[BOOK_HEADER_BYTES]);  // 0, or -1 when the hash refuses
// The whole check of zkr_book_blob_check.  0 and *h filled in, or -1 with `why` naming the first failure.
int book_blob_parse(const uint8_t *blob, size_t len, BookHeader *h, char *why, size_t why_len);

}  // namespace zkr
