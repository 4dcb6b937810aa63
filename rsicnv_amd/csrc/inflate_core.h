// inflate_core.h -- deflate (RFC 1951) decoding of one BGZF member's payload, with every bounds check, for the device
// inflate kernel (kernels_inflate.hip) and for plain host C++ (tests/sanitize_inflate, rsi_hot_inflate_bgzf's checks run
// on the device only).  The same functions run in both builds: on the device the 64 lanes of a wave execute the decode
// loop together with identical state (every lane reads the same bits and builds the same tables) and share the copy of
// a match and the stored bytes (lane / nlanes); on the host nlanes = 1.  Only lane 0 writes a literal.
//
// Memory safety on arbitrary input: every read of `in` is below `clen`, every write of `out` below `cap`, a distance is
// checked against the bytes produced, code-length sets that are over-subscribed or incomplete are refused (incomplete is
// allowed where zlib allows it: a single code of length 1, or no distance codes at all), and every loop is bounded by the
// input's bits or the output's bytes.  A bad member returns an Err code and writes nothing past `cap`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RSI_INF_HD __host__ __device__ inline
#else
#define RSI_INF_HD inline
#endif
// Before lanes read output bytes that other lanes wrote (a match copy after literals and earlier copies): the wave's LDS
// operations complete in order, and this keeps the compiler from moving them across each other.  Nothing on the host.
#if defined(__HIP_DEVICE_COMPILE__)
#define RSI_INF_LANE_SYNC() __builtin_amdgcn_wave_barrier()
#else
#define RSI_INF_LANE_SYNC() ((void)0)
#endif

namespace rsinf {

enum Err : int32_t {
  kOk = 0,
  kTruncated = 1,        // the payload ends inside a block
  kBadBlockType = 2,     // block type 3
  kStoredLen = 3,        // LEN != ~NLEN
  kBadCodeLengths = 4,   // over-subscribed / incomplete set, HLIT / HDIST out of range, a bad repeat, no end-of-block code
  kBadSymbol = 5,        // a bit pattern with no code, length symbol 286/287, distance symbol 30/31
  kDistTooFar = 6,       // a distance beyond the bytes produced
  kOutputOverrun = 7,    // more bytes than ISIZE
  kSizeMismatch = 8,     // fewer bytes than ISIZE
  kCrcMismatch = 9,      // CRC32 of the bytes != the footer's
  kTrailingData = 10,    // bytes left between the last deflate block and the footer
  kBadHeader = 11,       // (host) not a gzip / BGZF header, BSIZE too small, a block past the end of the file
};

RSI_INF_HD const char* err_name(int e) {
  switch (e) {
    case kOk: return "ok";
    case kTruncated: return "deflate data ends inside a block";
    case kBadBlockType: return "invalid deflate block type";
    case kStoredLen: return "stored block length check failed";
    case kBadCodeLengths: return "invalid Huffman code lengths";
    case kBadSymbol: return "invalid Huffman code";
    case kDistTooFar: return "distance too far back";
    case kOutputOverrun: return "more data than ISIZE";
    case kSizeMismatch: return "ISIZE mismatch";
    case kCrcMismatch: return "CRC32 mismatch";
    case kTrailingData: return "bytes between the deflate data and the footer";
    default: return "invalid BGZF header";
  }
}

// Canonical Huffman code (the counts per length and the symbols in code order), decoded length by length.
struct Huff {
  uint16_t count[16];
  uint16_t symbol[288];
};

// Scratch of one decode: in LDS on the device, shared by the lanes.
struct Work {
  Huff lit, dist;
  uint16_t lengths[320];
  uint16_t offs[16];
};

struct Bits {
  const uint8_t* in;
  uint32_t clen, pos;
  uint64_t buf;
  int cnt;
  RSI_INF_HD void refill() {
    while (cnt <= 56 && pos < clen) { buf |= (uint64_t)in[pos++] << cnt; cnt += 8; }
  }
  RSI_INF_HD bool get(int n, uint32_t& v) {   // n <= 16
    if (cnt < n) refill();
    if (cnt < n) return false;
    v = (uint32_t)(buf & ((1ull << n) - 1));
    buf >>= n; cnt -= n;
    return true;
  }
};

// Builds h from lengths[0..n).  Returns kOk, or kBadCodeLengths when the set is over-subscribed, or incomplete where not
// allowed: `may_be_empty` (distance codes) allows no code at all; one code of length 1 is always allowed (zlib's rules).
RSI_INF_HD int build(Huff& h, uint16_t* offs, const uint16_t* lengths, int n, bool may_be_empty) {
  for (int l = 0; l < 16; ++l) h.count[l] = 0;
  for (int s = 0; s < n; ++s) h.count[lengths[s]]++;   // lengths <= 15: the callers store nothing larger
  const int codes = n - h.count[0];
  if (codes == 0) return may_be_empty ? kOk : kBadCodeLengths;
  int left = 1;
  for (int l = 1; l < 16; ++l) {
    left <<= 1;
    left -= h.count[l];
    if (left < 0) return kBadCodeLengths;
  }
  if (left > 0 && !(codes == 1 && h.count[1] == 1)) return kBadCodeLengths;
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
  for (int s = 0; s < n; ++s) if (lengths[s]) h.symbol[offs[lengths[s]]++] = (uint16_t)s;
  return kOk;
}

// One symbol: < 0 on a pattern with no code (-kBadSymbol) or input that ends inside the code (-kTruncated).
RSI_INF_HD int decode(Bits& br, const Huff& h) {
  if (br.cnt < 15) br.refill();
  int code = 0, first = 0, index = 0;
  uint64_t b = br.buf;
  for (int l = 1; l < 16; ++l) {
    code |= (int)(b & 1);
    b >>= 1;
    const int count = h.count[l];
    if (code - count < first) {
      if (l > br.cnt) return -kTruncated;
      br.buf >>= l; br.cnt -= l;
      return h.symbol[index + (code - first)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return br.cnt < 15 ? -kTruncated : -kBadSymbol;
}

// RFC 1951 tables as arithmetic (no table to place in device memory)
RSI_INF_HD int len_base(int i) { return i < 8 ? 3 + i : (i == 28 ? 258 : ((4 + ((i - 4) & 3)) << ((i - 4) / 4)) + 3); }
RSI_INF_HD int len_extra(int i) { return i < 8 || i == 28 ? 0 : (i - 4) / 4; }
RSI_INF_HD int dist_base(int d) { return d < 4 ? 1 + d : ((2 + (d & 1)) << ((d - 2) / 2)) + 1; }
RSI_INF_HD int dist_extra(int d) { return d < 4 ? 0 : (d - 2) / 2; }
RSI_INF_HD int clen_order(int i) {
  if (i < 3) return 16 + i;
  const int j = i - 3;
  if (j == 0) return 0;
  const int k = (j + 1) / 2;
  return (j & 1) ? 7 + k : 8 - k;
}

// The literal/length and distance codes of one block into out[op..cap).
RSI_INF_HD int codes(Bits& br, const Work& w, uint8_t* out, uint32_t cap, uint32_t& op, int lane, int nlanes) {
  for (;;) {   // every pass consumes at least one bit and produces a byte, or ends the block
    const int sym = decode(br, w.lit);
    if (sym < 0) return -sym;
    if (sym < 256) {
      if (op >= cap) return kOutputOverrun;
      if (lane == 0) out[op] = (uint8_t)sym;
      ++op;
      continue;
    }
    if (sym == 256) return kOk;
    const int ls = sym - 257;
    if (ls >= 29) return kBadSymbol;
    uint32_t e = 0;
    if (!br.get(len_extra(ls), e)) return kTruncated;
    const uint32_t len = (uint32_t)len_base(ls) + e;
    const int ds = decode(br, w.dist);
    if (ds < 0) return -ds;
    if (ds >= 30) return kBadSymbol;
    if (!br.get(dist_extra(ds), e)) return kTruncated;
    const uint32_t dist = (uint32_t)dist_base(ds) + e;
    if (dist > op) return kDistTooFar;
    if (len > cap - op) return kOutputOverrun;
    // out[op + i] = out[op - dist + i % dist]: the same bytes as the byte-by-byte copy, with no lane reading a byte that
    // another lane writes in this copy
    const uint32_t src = op - dist;
    RSI_INF_LANE_SYNC();
    for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[op + i] = out[src + (dist >= len ? i : i % dist)];
    op += len;
  }
}

RSI_INF_HD int fixed_tables(Work& w) {
  for (int s = 0; s < 288; ++s) w.lengths[s] = s < 144 ? 8 : (s < 256 ? 9 : (s < 280 ? 7 : 8));
  if (build(w.lit, w.offs, w.lengths, 288, false) != kOk) return kBadCodeLengths;
  for (int s = 0; s < 32; ++s) w.lengths[s] = 5;   // 30 and 31 take part in the code but are invalid (codes() refuses them)
  return build(w.dist, w.offs, w.lengths, 32, false);
}

RSI_INF_HD int dynamic_tables(Bits& br, Work& w) {
  uint32_t hlit, hdist, hclen;
  if (!br.get(5, hlit) || !br.get(5, hdist) || !br.get(4, hclen)) return kTruncated;
  hlit += 257; hdist += 1; hclen += 4;
  if (hlit > 286 || hdist > 30) return kBadCodeLengths;
  for (int i = 0; i < 19; ++i) w.lengths[i] = 0;
  for (uint32_t i = 0; i < hclen; ++i) {
    uint32_t v;
    if (!br.get(3, v)) return kTruncated;
    w.lengths[clen_order((int)i)] = (uint16_t)v;
  }
  if (build(w.lit, w.offs, w.lengths, 19, false) != kOk) return kBadCodeLengths;
  // over-subscribed or incomplete code-length codes are refused above; a single length-1 code is let through as zlib does
  const uint32_t total = hlit + hdist;
  uint32_t index = 0;
  while (index < total) {   // every pass stores at least one length
    const int sym = decode(br, w.lit);
    if (sym < 0) return -sym;
    if (sym < 16) { w.lengths[index++] = (uint16_t)sym; continue; }
    uint16_t len = 0;
    uint32_t rep;
    if (sym == 16) {
      if (index == 0) return kBadCodeLengths;
      len = w.lengths[index - 1];
      if (!br.get(2, rep)) return kTruncated;
      rep += 3;
    } else if (sym == 17) {
      if (!br.get(3, rep)) return kTruncated;
      rep += 3;
    } else {
      if (!br.get(7, rep)) return kTruncated;
      rep += 11;
    }
    if (index + rep > total) return kBadCodeLengths;
    for (uint32_t r = 0; r < rep; ++r) w.lengths[index++] = len;
  }
  if (w.lengths[256] == 0) return kBadCodeLengths;
  if (build(w.lit, w.offs, w.lengths, (int)hlit, false) != kOk) return kBadCodeLengths;
  return build(w.dist, w.offs, w.lengths + hlit, (int)hdist, true);
}

// A raw deflate stream in[0..clen) into out[0..cap): *produced bytes.  The stream must use all of in[] (the BGZF footer
// follows it directly).
RSI_INF_HD int inflate_raw(const uint8_t* in, uint32_t clen, uint8_t* out, uint32_t cap, uint32_t* produced, Work& w,
                           int lane, int nlanes) {
  Bits br{in, clen, 0, 0, 0};
  uint32_t op = 0;
  *produced = 0;
  for (;;) {   // every block consumes at least 3 bits
    uint32_t hdr;
    if (!br.get(3, hdr)) return kTruncated;
    const uint32_t type = hdr >> 1;
    int rc = kOk;
    if (type == 0) {
      // byte-aligned: give back the whole bytes in the bit buffer, then LEN, NLEN and the bytes straight from in[]
      br.pos -= (uint32_t)(br.cnt >> 3);
      br.buf = 0; br.cnt = 0;
      if (clen - br.pos < 4) return kTruncated;
      const uint32_t len = (uint32_t)in[br.pos] | ((uint32_t)in[br.pos + 1] << 8);
      const uint32_t nlen = (uint32_t)in[br.pos + 2] | ((uint32_t)in[br.pos + 3] << 8);
      br.pos += 4;
      if (len != (~nlen & 0xffffu)) return kStoredLen;
      if (len > clen - br.pos) return kTruncated;
      if (len > cap - op) return kOutputOverrun;
      for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[op + i] = in[br.pos + i];
      RSI_INF_LANE_SYNC();
      br.pos += len; op += len;
    } else if (type == 1) {
      rc = fixed_tables(w);
      if (rc == kOk) rc = codes(br, w, out, cap, op, lane, nlanes);
    } else if (type == 2) {
      rc = dynamic_tables(br, w);
      if (rc == kOk) rc = codes(br, w, out, cap, op, lane, nlanes);
    } else {
      return kBadBlockType;
    }
    if (rc != kOk) return rc;
    if (hdr & 1) break;
  }
  *produced = op;
  if (br.pos - (uint32_t)(br.cnt >> 3) != clen) return kTrailingData;
  return kOk;
}

// ---- CRC32 (the gzip polynomial, reflected), and combining the CRCs of pieces: crc(A B) = crc(A) * x^(8|B|) + crc(B) ----
constexpr uint32_t kPoly = 0xedb88320u;

RSI_INF_HD uint32_t crc32(uint32_t crc, const uint8_t* p, uint32_t n) {
  crc = ~crc;
  for (uint32_t i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (kPoly & (0u - (crc & 1u)));
  }
  return ~crc;
}

RSI_INF_HD uint32_t multmodp(uint32_t a, uint32_t b) {   // a * b mod p, polynomials bit-reflected
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1)) == 0) break;
    }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}

// x2n[k] = x^(2^k) mod p, k < 32: the shift constants (computed once on the host, read by the device from constant memory)
struct X2n { uint32_t v[32]; };
inline X2n make_x2n() {
  X2n t{};
  uint32_t p = 1u << 30;   // x^1
  t.v[0] = p;
  for (int k = 1; k < 32; ++k) t.v[k] = p = multmodp(p, p);
  return t;
}

RSI_INF_HD uint32_t shift_bytes(const uint32_t* x2n, uint32_t crc, uint32_t nbytes) {   // crc * x^(8 nbytes) mod p
  uint32_t p = 1u << 31;   // x^0
  int k = 3;
  while (nbytes) {
    if (nbytes & 1) p = multmodp(x2n[k & 31], p);
    nbytes >>= 1;
    ++k;
  }
  return multmodp(p, crc);
}

}  // namespace rsinf

namespace rsinf {

// ---- BGZF member headers (host): gzip ID, CM = 8, FLG = FEXTRA only, a "BC" subfield of length 2 holding BSIZE - 1 ----
struct Member {
  uint32_t bsize;   // whole member, header to footer
  uint32_t hdr;     // bytes in front of the deflate payload
  uint32_t clen;    // deflate payload
  uint32_t crc, isize;
};

// 1: a BGZF member header starts p (m filled; crc / isize only when avail >= bsize); 0: not BGZF; -1: fewer than the
// header's bytes available
inline int bgzf_member(const uint8_t* p, size_t avail, Member& m) {
  if (avail < 12) return avail >= 4 && !(p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && p[3] == 4) ? 0 : -1;
  if (!(p[0] == 0x1f && p[1] == 0x8b && p[2] == 8 && p[3] == 4)) return 0;
  const uint32_t xlen = (uint32_t)p[10] | ((uint32_t)p[11] << 8);
  if (avail < 12 + (size_t)xlen) return -1;
  uint32_t bsize = 0;
  for (uint32_t k = 0; k + 4 <= xlen;) {   // the subfields
    const uint8_t* s = p + 12 + k;
    const uint32_t slen = (uint32_t)s[2] | ((uint32_t)s[3] << 8);
    if (s[0] == 'B' && s[1] == 'C' && slen == 2 && k + 6 <= xlen) bsize = ((uint32_t)s[4] | ((uint32_t)s[5] << 8)) + 1;
    k += 4 + slen;
  }
  if (bsize == 0) return 0;
  m.bsize = bsize; m.hdr = 12 + xlen;
  if (bsize < m.hdr + 8) return 0;
  m.clen = bsize - m.hdr - 8;
  m.crc = m.isize = 0;
  if (avail >= bsize) {
    const uint8_t* f = p + bsize - 8;
    m.crc = (uint32_t)f[0] | ((uint32_t)f[1] << 8) | ((uint32_t)f[2] << 16) | ((uint32_t)f[3] << 24);
    m.isize = (uint32_t)f[4] | ((uint32_t)f[5] << 8) | ((uint32_t)f[6] << 16) | ((uint32_t)f[7] << 24);
  }
  return 1;
}

// The format of a depth file from its first bytes: 0 text, 1 BGZF, 2 gzip
inline int detect_format(const uint8_t* p, size_t n) {
  if (n < 2 || p[0] != 0x1f || p[1] != 0x8b) return 0;
  Member m;
  return bgzf_member(p, n, m) == 1 ? 1 : 2;
}

}  // namespace rsinf
