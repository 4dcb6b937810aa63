// deflate_core.h -- one block of text (at most 65280 bytes, a BGZF member's worth) to a raw deflate stream (RFC 1951), for the
// device kernel (kernels_deflate.hip) and for plain host C++ (tests/sanitize_deflate).  The same functions run in both builds:
// on the device the `nlanes` threads of a workgroup share the work between barriers, on the host nlanes = 1 and a barrier is
// nothing.  Every lane calls every function with the same arguments (the control flow around barriers is uniform).
//
// The stream is a sequence of dynamic-Huffman blocks (BTYPE = 10), one per kBlock text bytes, each with codes built from its own
// token histogram; a stream that would not be shorter than the stored form (len + 5 bytes) is replaced by one stored block.
//
// The bytes are a function of the text alone.  The match candidate of position p is the NEAREST EARLIER position with the same
// hash of text[p, p + 3), if it lies at most 32768 back: a definition by position, whatever the lane count (positions are worked
// through in steps of nlanes; inside a step a lane finds its candidate among the step's hashes, else in the table the steps
// before left, and the last position of a step with a hash writes the table).  Counts are sums, the output bits are OR-ed into
// zeroed memory: neither depends on an order.
//
// Memory safety: every read of `text` is below `len`, every write of `out` below min(cap, len + 5), every loop is bounded by len.
#pragma once
#include "inflate_core.h"   // the RFC 1951 length / distance tables, clen_order, CRC32

#if defined(__HIP_DEVICE_COMPILE__)
#define RSI_DEF_SYNC() __syncthreads()
#define RSI_DEF_ADD(p, v) ((void)atomicAdd((p), (v)))
#else
#define RSI_DEF_SYNC() ((void)0)
#define RSI_DEF_ADD(p, v) ((void)(*(p) += (v)))
#endif

namespace rsdef {

constexpr uint32_t kMaxText = 65280;    // text bytes of one BGZF member (bgzip's block size)
constexpr uint32_t kBlock = 16384;      // text bytes of one deflate block: what its tokens' storage holds
constexpr int kHashBits = 14;
constexpr uint32_t kNone = 0xffffu;     // no position (positions are below kMaxText)
constexpr uint32_t kWindow = 32768;
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kFarShort = 4096;    // a match of 3 bytes further back than this costs more than its literals
constexpr int kMaxLanes = 256;
constexpr int kLitSyms = 286, kDistSyms = 30, kClenSyms = 19;
constexpr uint32_t kBgzfHeader = 18, kBgzfFooter = 8;
constexpr uint32_t kSlotBytes = 65536;  // a member's slot: header, payload (at most kMaxText + 5), footer

// Scratch of one member: in LDS on the device (beside the 65280 bytes of text), shared by the lanes.
struct Work {
  uint16_t table[1u << kHashBits];   // last position seen with a hash
  uint16_t mdist[kBlock];            // per position of the block: distance of its match, 0 = none
  uint8_t mlen[kBlock];              // its length - 3
  uint32_t tok[kBlock / 32];         // bit i: position i starts a token (the greedy walk came by)
  union {
    uint16_t hs[kMaxLanes];           // the hashes of one step (kNone where the step has no position or the position no hash)
    uint32_t hs_pairs[kMaxLanes / 2];
  };
  uint32_t lane_bits[kMaxLanes];     // bit offset of each lane's first token
  uint32_t lit_cnt[288], dist_cnt[32], cl_cnt[20];
  uint16_t lit_code[288], dist_code[32], cl_code[20];   // bit-reversed: ready to be OR-ed in
  uint8_t lit_len[288], dist_len[32], cl_len[20];
  // code construction
  uint16_t order[288], leaf_parent[288], node_parent[288];
  uint32_t node_weight[288];
  uint8_t node_depth[288];
  uint32_t carry;      // where the greedy walk goes on (the end of the last token)
  uint32_t bitpos;     // bits of the stream so far
  uint32_t hlit, hdist, hclen;
  uint32_t give_up;    // the coded stream would not be shorter than the stored one
};

RSI_INF_HD uint32_t hash3(const uint8_t* t) {
  return ((uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16)) * 0x9e3779b1u >> (32 - kHashBits);
}
RSI_INF_HD int ilog2(uint32_t x) { return 31 - __builtin_clz(x); }   // x > 0
RSI_INF_HD int len_code(uint32_t len) {                              // 3 .. 258 -> 0 .. 28 (symbol 257 + code)
  if (len == kMaxMatch) return 28;
  const uint32_t x = len - 3;
  if (x < 4) return (int)x;
  const int e = ilog2(x) - 2;
  return 4 + 4 * e + (int)(x >> e) - 4;
}
RSI_INF_HD int dist_code(uint32_t dist) {                            // 1 .. 32768 -> 0 .. 29
  const uint32_t x = dist - 1;
  if (x < 4) return (int)x;
  const int e = ilog2(x) - 1;
  return 2 + 2 * e + (int)(x >> e) - 2;
}
RSI_INF_HD uint32_t reverse_bits(uint32_t c, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) { r = (r << 1) | (c & 1u); c >>= 1; }
  return r;
}

// n <= 57 bits of v (nothing above them) into the stream at bit `pos`: OR into zeroed bytes
RSI_INF_HD void put_bits(uint8_t* out, uint32_t pos, uint64_t v, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  // whole 32-bit words of the slot; a word without a bit of v is left alone
  const uintptr_t a = reinterpret_cast<uintptr_t>(out);
  unsigned int* base = reinterpret_cast<unsigned int*>(a & ~uintptr_t(3));
  const uint32_t bp = pos + (uint32_t)(a & 3) * 8;
  const uint32_t wi = bp >> 5, sh = bp & 31;
  const uint64_t lo = v << sh;
  const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
  if (w0) atomicOr(base + wi, w0);
  if (w1) atomicOr(base + wi + 1, w1);
  if (w2) atomicOr(base + wi + 2, w2);
  (void)n;
#else
  uint32_t byte = pos >> 3;
  int sh = (int)(pos & 7);
  while (n > 0) {
    out[byte++] |= (uint8_t)(v << sh);
    v >>= 8 - sh;
    n -= 8 - sh;
    sh = 0;
  }
#endif
}

// Code lengths of at most maxbits for cnt[0, n), and their canonical codes (bit-reversed).  A symbol that does not occur gets
// length 0; one used symbol gets length 1 (the caller sees to it that this is allowed); two or more give a complete set: the
// Huffman lengths (two queues over the symbols sorted by count, ties by symbol), then lengths above maxbits are cut to it and
// the Kraft sum is brought back to 1 by lengthening the longest shorter codes, and the lengths go to the symbols by count.
RSI_INF_HD void build_codes(const uint32_t* cnt, int n, int maxbits, uint8_t* len, uint16_t* code, Work& w, int lane, int nlanes) {
  for (int s = lane; s < n; s += nlanes) {
    len[s] = 0;
    code[s] = 0;
    const uint32_t c = cnt[s];
    if (c == 0) continue;
    int rank = 0;
    for (int t = 0; t < n; ++t) {
      const uint32_t ct = cnt[t];
      rank += (ct != 0 && (ct < c || (ct == c && t < s))) ? 1 : 0;
    }
    w.order[rank] = (uint16_t)s;
  }
  RSI_DEF_SYNC();
  if (lane == 0) {
    int used = 0;
    for (int s = 0; s < n; ++s) used += cnt[s] != 0 ? 1 : 0;
    uint32_t num[33];
    for (int l = 0; l < 33; ++l) num[l] = 0;
    if (used == 1) {
      num[1] = 1;
    } else if (used > 1) {
      int li = 0, ni = 0;   // next leaf, next unmerged node
      for (int k = 0; k < used - 1; ++k) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
          const bool leaf = li < used && (ni >= k || cnt[w.order[li]] <= w.node_weight[ni]);
          if (leaf) { sum += cnt[w.order[li]]; w.leaf_parent[li++] = (uint16_t)k; }
          else { sum += w.node_weight[ni]; w.node_parent[ni++] = (uint16_t)k; }
        }
        w.node_weight[k] = sum;
      }
      w.node_depth[used - 2] = 0;
      for (int k = used - 3; k >= 0; --k) {
        const int d = w.node_depth[w.node_parent[k]] + 1;
        w.node_depth[k] = (uint8_t)(d > 32 ? 32 : d);   // beyond maxbits all the same
      }
      for (int k = 0; k < used; ++k) {
        const int d = w.node_depth[w.leaf_parent[k]] + 1;
        num[d > 32 ? 32 : d]++;
      }
      for (int l = maxbits + 1; l < 33; ++l) { num[maxbits] += num[l]; num[l] = 0; }
      uint32_t total = 0;
      for (int l = maxbits; l > 0; --l) total += num[l] << (maxbits - l);
      while (total > (1u << maxbits)) {   // each pass takes 1 off the sum
        num[maxbits]--;
        for (int l = maxbits - 1; l > 0; --l) if (num[l]) { num[l]--; num[l + 1] += 2; break; }
        total--;
      }
    }
    // the most frequent symbol gets the shortest length
    int k = used - 1;
    for (int l = 1; l <= maxbits; ++l) for (uint32_t j = 0; j < num[l] && k >= 0; ++j) len[w.order[k--]] = (uint8_t)l;
    uint32_t next[17], c = 0;
    next[0] = 0;
    for (int l = 1; l <= maxbits; ++l) { c = (c + (l > 1 ? num[l - 1] : 0)) << 1; next[l] = c; }
    for (int s = 0; s < n; ++s) if (len[s]) code[s] = (uint16_t)reverse_bits(next[len[s]]++, len[s]);
  }
  RSI_DEF_SYNC();
}

// One token's bits: a literal, or length code + extra, distance code + extra (at most 15 + 5 + 15 + 13)
RSI_INF_HD int token_bits(const Work& w, const uint8_t* text, uint32_t s, uint32_t i, uint64_t& v) {
  const uint32_t d = w.mdist[i];
  if (d == 0) {
    const int c = text[s + i];
    v = w.lit_code[c];
    return w.lit_len[c];
  }
  const uint32_t l = (uint32_t)w.mlen[i] + 3;
  const int lc = len_code(l), dc = dist_code(d);
  int n = w.lit_len[257 + lc];
  v = w.lit_code[257 + lc];
  v |= (uint64_t)(l - (uint32_t)rsinf::len_base(lc)) << n;
  n += rsinf::len_extra(lc);
  v |= (uint64_t)w.dist_code[dc] << n;
  n += w.dist_len[dc];
  v |= (uint64_t)(d - (uint32_t)rsinf::dist_base(dc)) << n;
  n += rsinf::dist_extra(dc);
  return n;
}

RSI_INF_HD bool is_token(const Work& w, uint32_t i) { return (w.tok[i >> 5] >> (i & 31)) & 1u; }

// text[0, len), len <= kMaxText, as a raw deflate stream into out[0, cap).  Returns its bytes (the same in every lane), 0 when
// len == 0, len > kMaxText or cap < len + 5 (nothing written); *stored: 1 when it is one stored block.
RSI_INF_HD uint32_t deflate_raw(const uint8_t* text, uint32_t len, uint8_t* out, uint32_t cap, Work& w, int lane, int nlanes,
                                int* stored) {
  *stored = 0;
  if (len == 0 || len > kMaxText || cap < len + 5 || nlanes > kMaxLanes) return 0;
  const uint32_t limit = len + 5;   // the stored form
  for (uint32_t i = (uint32_t)lane; i < limit; i += (uint32_t)nlanes) out[i] = 0;
  for (uint32_t i = (uint32_t)lane; i < (1u << kHashBits); i += (uint32_t)nlanes) w.table[i] = (uint16_t)kNone;
  if (lane == 0) { w.carry = 0; w.bitpos = 0; w.give_up = 0; }
  RSI_DEF_SYNC();

  for (uint32_t s = 0; s < len; s += kBlock) {   // one deflate block
    const uint32_t e = s + kBlock < len ? s + kBlock : len;
    const uint32_t npos = e - s;
    // ---- every position's candidate and match ----
    for (uint32_t i = (uint32_t)lane; i < kBlock / 32; i += (uint32_t)nlanes) w.tok[i] = 0;
    for (uint32_t base = s; base < e; base += (uint32_t)nlanes) {
      const uint32_t p = base + (uint32_t)lane;
      const uint32_t h = (p < e && p + 2 < len) ? hash3(text + p) : kNone;
      w.hs[lane] = (uint16_t)h;
      RSI_DEF_SYNC();
      // the nearest earlier position of the step with this hash, and whether a later one has it: every lane wrote hs[], and
      // every lane looks at all of it without a branch (two hashes a word)
      int near = -1;
      uint32_t later = 0;
      if (nlanes % 2 == 0) {
        const uint32_t* pairs = w.hs_pairs;   // (little-endian: hs[j] is the low half of pair j / 2)
        for (int j = 0; j < nlanes; j += 2) {
          const uint32_t q = pairs[j >> 1];
          const bool e0 = (q & 0xffffu) == h, e1 = (q >> 16) == h;
          near = e0 && j < lane ? j : near;
          near = e1 && j + 1 < lane ? j + 1 : near;
          later |= (uint32_t)(e0 && j > lane) | (uint32_t)(e1 && j + 1 > lane);
        }
      }
      uint32_t cand = kNone;
      const bool last = later == 0;
      if (h != kNone) cand = near >= 0 ? base + (uint32_t)near : w.table[h];
      RSI_DEF_SYNC();   // the table is read: now the step's positions enter it
      if (h != kNone && last) w.table[h] = (uint16_t)p;
      if (p < e) {
        uint32_t ml = 0, md = 0;
        if (cand != kNone && p - cand <= kWindow) {
          const uint32_t maxl = len - p < kMaxMatch ? len - p : kMaxMatch;
          uint32_t l = 0;
          while (l < maxl && text[cand + l] == text[p + l]) ++l;
          if (l >= kMinMatch && !(l == kMinMatch && p - cand > kFarShort)) { ml = l; md = p - cand; }
        }
        w.mdist[p - s] = (uint16_t)md;
        w.mlen[p - s] = (uint8_t)(md ? ml - 3 : 0);
      }
    }
    for (int i = lane; i < 288; i += nlanes) w.lit_cnt[i] = i == 256 ? 1u : 0u;   // one end-of-block
    for (int i = lane; i < 32; i += nlanes) w.dist_cnt[i] = 0;
    for (int i = lane; i < 20; i += nlanes) w.cl_cnt[i] = 0;
    RSI_DEF_SYNC();
    // ---- the greedy walk: which positions start a token ----
    if (lane == 0) {
      uint32_t p = w.carry, word = kNone, bits = 0;   // the bits of one word of tok[] are collected, then stored (tok[] is zero)
      while (p < e) {   // p grows by at least 1
        const uint32_t i = p - s;
        if ((i >> 5) != word) {
          if (word != kNone) w.tok[word] = bits;
          word = i >> 5; bits = 0;
        }
        bits |= 1u << (i & 31);
        const uint32_t d = w.mdist[i], l = w.mlen[i];   // both read at once: one LDS round trip a token
        p += d ? l + 3 : 1u;
      }
      if (word != kNone) w.tok[word] = bits;
      w.carry = p;   // <= len: no match passes the text's end
    }
    RSI_DEF_SYNC();
    const bool final_block = w.carry >= len;
    // ---- the block's histogram and codes ----
    for (uint32_t i = (uint32_t)lane; i < npos; i += (uint32_t)nlanes) {
      if (!is_token(w, i)) continue;
      const uint32_t d = w.mdist[i];
      if (d == 0) { RSI_DEF_ADD(&w.lit_cnt[text[s + i]], 1u); continue; }
      RSI_DEF_ADD(&w.lit_cnt[257 + len_code((uint32_t)w.mlen[i] + 3)], 1u);
      RSI_DEF_ADD(&w.dist_cnt[dist_code(d)], 1u);
    }
    RSI_DEF_SYNC();
    build_codes(w.lit_cnt, kLitSyms, 15, w.lit_len, w.lit_code, w, lane, nlanes);
    build_codes(w.dist_cnt, kDistSyms, 15, w.dist_len, w.dist_code, w, lane, nlanes);
    if (lane == 0) {
      int hlit = kLitSyms, hdist = kDistSyms;
      while (hlit > 257 && w.lit_len[hlit - 1] == 0) --hlit;
      while (hdist > 1 && w.dist_len[hdist - 1] == 0) --hdist;
      if (hdist == 1 && w.dist_len[0] == 0) w.dist_len[0] = 1;   // no distance code: one of length 1 that is never used
      w.hlit = (uint32_t)hlit; w.hdist = (uint32_t)hdist;
      for (int i = 0; i < hlit; ++i) w.cl_cnt[w.lit_len[i]]++;
      for (int i = 0; i < hdist; ++i) w.cl_cnt[w.dist_len[i]]++;
      int used = 0, one = 0;
      for (int i = 0; i < kClenSyms; ++i) if (w.cl_cnt[i]) { ++used; one = i; }
      if (used < 2) w.cl_cnt[one == 0 ? 1 : 0] = 1;   // the code-length code must be complete: a second symbol, never sent
    }
    RSI_DEF_SYNC();
    build_codes(w.cl_cnt, kClenSyms, 7, w.cl_len, w.cl_code, w, lane, nlanes);
    // ---- the block's size, before a bit is written ----
    if (lane == 0) {
      int hclen = kClenSyms;
      while (hclen > 4 && w.cl_len[rsinf::clen_order(hclen - 1)] == 0) --hclen;
      w.hclen = (uint32_t)hclen;
      uint64_t bits = 3 + 5 + 5 + 4 + 3 * (uint64_t)hclen;
      for (uint32_t i = 0; i < w.hlit; ++i) bits += w.cl_len[w.lit_len[i]];
      for (uint32_t i = 0; i < w.hdist; ++i) bits += w.cl_len[w.dist_len[i]];
      for (int i = 0; i < kLitSyms; ++i) bits += (uint64_t)w.lit_cnt[i] * (w.lit_len[i] + (i > 256 ? (uint32_t)rsinf::len_extra(i - 257) : 0u));
      for (int i = 0; i < kDistSyms; ++i) bits += (uint64_t)w.dist_cnt[i] * (w.dist_len[i] + (uint32_t)rsinf::dist_extra(i));
      if ((w.bitpos + bits + 7) / 8 >= limit) w.give_up = 1;
    }
    RSI_DEF_SYNC();
    if (w.give_up) break;
    // ---- header (lane 0), then every lane the tokens of its stretch of positions ----
    const uint32_t per = (npos + (uint32_t)nlanes - 1) / (uint32_t)nlanes;
    const uint32_t i0 = (uint32_t)lane * per < npos ? (uint32_t)lane * per : npos;
    const uint32_t i1 = i0 + per < npos ? i0 + per : npos;
    {
      uint32_t mine = 0;
      for (uint32_t i = i0; i < i1; ++i) {
        if (!is_token(w, i)) continue;
        uint64_t v;
        mine += (uint32_t)token_bits(w, text, s, i, v);
      }
      w.lane_bits[lane] = mine;
    }
    RSI_DEF_SYNC();
    if (lane == 0) {
      uint32_t pos = w.bitpos;
      put_bits(out, pos, (final_block ? 1u : 0u) | (2u << 1), 3); pos += 3;
      put_bits(out, pos, w.hlit - 257, 5); pos += 5;
      put_bits(out, pos, w.hdist - 1, 5); pos += 5;
      put_bits(out, pos, w.hclen - 4, 4); pos += 4;
      for (uint32_t i = 0; i < w.hclen; ++i) { put_bits(out, pos, w.cl_len[rsinf::clen_order((int)i)], 3); pos += 3; }
      for (uint32_t i = 0; i < w.hlit + w.hdist; ++i) {   // every length spelled out: no repeat codes
        const int l = i < w.hlit ? w.lit_len[i] : w.dist_len[i - w.hlit];
        put_bits(out, pos, w.cl_code[l], w.cl_len[l]);
        pos += w.cl_len[l];
      }
      for (int k = 0; k < nlanes; ++k) { const uint32_t b = w.lane_bits[k]; w.lane_bits[k] = pos; pos += b; }
      put_bits(out, pos, w.lit_code[256], w.lit_len[256]);
      w.bitpos = pos + w.lit_len[256];
    }
    RSI_DEF_SYNC();
    {
      uint32_t pos = w.lane_bits[lane];
      for (uint32_t i = i0; i < i1; ++i) {
        if (!is_token(w, i)) continue;
        uint64_t v;
        const int n = token_bits(w, text, s, i, v);
        put_bits(out, pos, v, n);
        pos += (uint32_t)n;
      }
    }
    RSI_DEF_SYNC();
    if (final_block) break;
  }
  if (!w.give_up) return (w.bitpos + 7) / 8;
  // ---- stored: BFINAL = 1, BTYPE = 00, LEN, ~LEN, the bytes ----
  RSI_DEF_SYNC();
  *stored = 1;
  if (lane == 0) {
    out[0] = 1;
    out[1] = (uint8_t)(len & 0xff); out[2] = (uint8_t)(len >> 8);
    out[3] = (uint8_t)(~len & 0xff); out[4] = (uint8_t)((~len >> 8) & 0xff);
  }
  for (uint32_t i = (uint32_t)lane; i < len; i += (uint32_t)nlanes) out[5 + i] = text[i];
  RSI_DEF_SYNC();
  return limit;
}

// ---- the BGZF frame around a payload (lane 0): 18 bytes in front, CRC32 and ISIZE behind ----
RSI_INF_HD void bgzf_frame(uint8_t* member, uint32_t payload, uint32_t crc, uint32_t isize) {
  const uint32_t bsize1 = kBgzfHeader + payload + kBgzfFooter - 1;
  const uint8_t h[kBgzfHeader] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)(bsize1 & 0xff), (uint8_t)(bsize1 >> 8)};
  for (uint32_t i = 0; i < kBgzfHeader; ++i) member[i] = h[i];
  uint8_t* f = member + kBgzfHeader + payload;
  for (int k = 0; k < 4; ++k) { f[k] = (uint8_t)(crc >> (8 * k)); f[4 + k] = (uint8_t)(isize >> (8 * k)); }
}

}  // namespace rsdef
