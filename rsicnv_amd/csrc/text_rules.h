// text_rules.h -- the depth-text readers' integer extraction: what the reference's `istringstream iss(line); iss >> pos >> d`
// (load_data_from_text, loaddata.cpp:496-517) does with libstdc++, for the device parse kernels (kernels_io.hip), the host
// fallback loop (parse_depth_text_host in ingest.hip) and plain host C++ (tests/sanitize_text checks it against
// std::istringstream under ASan + UBSan).  DESIGN.md 6c / 6d state the line rules built on it.
//
// One extraction on [q, e), q left behind what it consumed:
// * skip the blanks ' ' \t \r \v \f (the C locale's isspace; lines never hold '\n');
// * an optional '+' or '-', then a run of digits; without a digit the extraction fails and gives 0;
// * a value outside the field's type fails and gives the nearest bound: libstdc++ reads an `int` through `long` and clamps,
//   so a 32-bit field gives INT_MAX / INT_MIN however far out the digits go, a 64-bit field LLONG_MAX / LLONG_MIN.
// After a failed extraction the stream has failed: the later extractions of the line leave their (zero-initialised)
// variables alone, so the callers read no further.  A stream that reaches the end of the line while skipping blanks fails
// in the same way with the variable untouched, which for a zero-initialised variable is the 0 given here.
//
// The digits accumulate in an unsigned magnitude that saturates: above kCut another digit gives kSat, which stays put; at
// or below it, x * 10 + 9 fits.  No signed arithmetic can overflow, and the cost per digit is one compare and a select.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RSI_TXT_HD __host__ __device__ inline
#else
#define RSI_TXT_HD inline
#endif

namespace rsitxt {

RSI_TXT_HD bool is_blank(unsigned char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f'; }

// U: the magnitude's type (uint32_t for 32-bit fields, uint64_t for 64-bit ones); kMag = 2^(bits - 1), the largest negative
// magnitude.  kCut = kMag / 10, so x <= kCut gives x * 10 + 9 <= kMag + 9 < 2^bits; kSat = kMag + 1 marks an overflow.
template <typename U, U kMag, typename Ch>
RSI_TXT_HD bool extract(const Ch* t, long long& q, long long e, long long& v) {
  constexpr U kCut = kMag / 10, kSat = kMag + 1;
  while (q < e && is_blank((unsigned char)t[q])) ++q;
  bool neg = false;
  if (q < e && (t[q] == '-' || t[q] == '+')) { neg = t[q] == '-'; ++q; }
  if (q >= e || (unsigned)((unsigned char)t[q] - '0') > 9u) { v = 0; return false; }
  U x = 0;
  for (; q < e; ++q) {
    const unsigned dg = (unsigned)((unsigned char)t[q] - '0');
    if (dg > 9u) break;
    x = x > kCut ? kSat : (U)(x * 10u + dg);
  }
  if (neg) {
    if (x > kMag) { v = -(long long)(kMag - 1) - 1; return false; }
    v = x == kMag ? -(long long)(kMag - 1) - 1 : -(long long)x;
    return true;
  }
  if (x > kMag - 1) { v = (long long)(kMag - 1); return false; }
  v = (long long)x;
  return true;
}

// `iss >> v` into an int (pos, d and the cohort columns) and into a long long (bedGraph start and end).
template <typename Ch>
RSI_TXT_HD bool extract_i32(const Ch* t, long long& q, long long e, long long& v) {
  return extract<uint32_t, (uint32_t)1 << 31>(t, q, e, v);
}
template <typename Ch>
RSI_TXT_HD bool extract_i64(const Ch* t, long long& q, long long e, long long& v) {
  return extract<uint64_t, (uint64_t)1 << 63>(t, q, e, v);
}

}  // namespace rsitxt
