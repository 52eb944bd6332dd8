// pco_verify.h -- the verdict on one task of a verified encode (include/pco_gfx.h section 3b: PCO_GFX_CFG_VERIFY, pco_gfx_verify_chunks,
// pco_gfx_verify_wrapped_chunks): what the encode left, what the decode of those bytes ended with and where the compare kernel found the first
// difference, turned into the task's result.  Plain C++ without a device header, so that verify_finish_kernel (verify.hip) and a CPU test
// (tests/test_verify_abi.py compiles it with g++) run the same lines.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PCO_VERIFY_HD __host__ __device__
#else
#define PCO_VERIFY_HD
#endif

namespace pcogfx {

constexpr uint32_t kVerifyOk = 0, kVerifyCorruption = 1;   // enum PcoGfxStatus: PCO_GFX_OK, PCO_GFX_CORRUPTION
constexpr uint32_t kVerifyAuxVerified = 2;                 // PCO_GFX_AUX_VERIFIED
constexpr uint64_t kVerifyNoDifference = ~(uint64_t)0;     // what the first-difference word is initialised to

struct VerifyResult { uint64_t n_out, consumed; uint32_t status, aux; };   // PcoGfxTaskResult's fields in its order

// enc: the task's encode result.  dec_status / dec_n_out: how the decode of the bytes ended and how many numbers it wrote.  n: the task's count
// of numbers.  first: the lowest index at which a decoded number differs from its source among the first min(dec_n_out, n), or
// kVerifyNoDifference; an index at or behind that count names nothing that was compared and is ignored.
//   encode not OK                       the result as it is: nothing of the task was decoded or compared
//   decode not OK                       Corruption, n_out 0, consumed ~0
//   a difference at `first`             Corruption, n_out 0, consumed first
//   no difference, dec_n_out < n        Corruption, n_out 0, consumed dec_n_out
//   no difference, dec_n_out > n        Corruption, n_out 0, consumed n (the first index the source does not have)
//   no difference, dec_n_out == n       the encode result with PCO_GFX_AUX_VERIFIED set
// A failed verdict keeps aux bit 0 (the chunk fell back) and clears bit 1.
PCO_VERIFY_HD inline VerifyResult verify_verdict(VerifyResult enc, uint32_t dec_status, uint64_t dec_n_out, uint64_t n, uint64_t first) {
  if (enc.status != kVerifyOk) return enc;
  VerifyResult bad{0, kVerifyNoDifference, kVerifyCorruption, enc.aux & ~kVerifyAuxVerified};
  if (dec_status != kVerifyOk) return bad;
  const uint64_t compared = dec_n_out < n ? dec_n_out : n;
  if (first < compared) { bad.consumed = first; return bad; }
  if (dec_n_out != n) { bad.consumed = compared; return bad; }
  enc.aux |= kVerifyAuxVerified;
  return enc;
}

}  // namespace pcogfx
