// Host-only check of sp_lbo_check_partition (csrc/sp_lbo.hip), the half of sp_lbo_read_partition that needs no device:
// the partition sp_lbo_ensemble and sp_lbo_linear take is e_0 = 0, e_nblocks = K, every width in 1 .. SP_LBO_R = 64; the
// widest block and the number of bands come back for a partition that passes and stay untouched for one that does not.
// No GPU, no python: `make -C starry_process_amd/csrc check-partition` builds it with ASan and UBSan on the host pass
// and runs it (prints "ok: N checks", exit status 0).  Every edge list is a heap array of exactly nblocks + 1 entries, so
// a read past either end is the sanitizer's finding.
#include <cstdio>
#include <vector>

#include "../starry_process_amd/csrc/sp_internal.h"

static int nchecks = 0, nfail = 0;
#define CHECK(cond)                                         \
  do {                                                      \
    ++nchecks;                                              \
    if (!(cond)) {                                          \
      ++nfail;                                              \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                       \
  } while (0)

// rc of the check and, where it passes, bmax and nbands; -7 marks a result the function must not have written
static void expect(std::vector<int32_t> e, int K, int rc, int bmax, int nbands) {
  int got_bmax = -7, got_nbands = -7;
  const int nblocks = (int)e.size() - 1;
  CHECK(sp_lbo_check_partition(e.data(), nblocks, K, &got_bmax, &got_nbands) == rc);
  CHECK(got_bmax == (rc ? -7 : bmax));
  CHECK(got_nbands == (rc ? -7 : nbands));
  if (!rc) CHECK(got_nbands == sp_lbo_count_bands(e.data(), nblocks));
}

int main() {
  static_assert(SP_LBO_R == 64, "the widest block the band kernel holds");
  const int Ks[5] = {2, 64, 65, 130, 1000};
  for (int K : Ks) {
    expect({0, K}, K, K <= 64 ? SP_OK : SP_ERR_INVALID, K, 1);
    if (K > 64) {
      expect({0, 64, K}, K, K - 64 <= 64 ? SP_OK : SP_ERR_INVALID, 64, 2);
      expect({0, 65, K}, K, SP_ERR_INVALID, 0, 0);       // (one cadence too wide)
    }
    expect({1, K}, K, SP_ERR_INVALID, 0, 0);             // (does not start at 0)
    expect({0, K - 1}, K, SP_ERR_INVALID, 0, 0);         // (does not end at K)
    expect({0, 1, 1, K}, K, SP_ERR_INVALID, 0, 0);       // (a block of no cadence)
    expect({0, K, K}, K, SP_ERR_INVALID, 0, 0);
    expect({0, 1, 0, K}, K, SP_ERR_INVALID, 0, 0);       // (edges that go back)
  }
  // single cadences: 64 of them fill a band
  for (int K : {2, 64, 65, 129}) {
    std::vector<int32_t> e(K + 1);
    for (int j = 0; j <= K; ++j) e[j] = j;
    expect(e, K, SP_OK, 1, (K + 63) / 64);
  }
  // a band closes where the next block would pass 64 rows: widths 40, 24 | 25, 39 | 1
  expect({0, 40, 64, 89, 128, 129}, 129, SP_OK, 40, 3);
  expect({0, 40, 65, 129}, 129, SP_OK, 64, 3);           // widths 40 | 25 | 64
  if (nfail) std::printf("FAILED: %d of %d checks\n", nfail, nchecks);
  else std::printf("ok: %d checks\n", nchecks);
  return nfail ? 1 : 0;
}
