// Arithmetic of the SNAP text (.net) ingest (sheep_ingest.hip, net_pass in sheep_capi.cpp): the
// byte classes, the token-start mask of a 16-byte word, the parse of one token, where the host
// cuts a chunk, and which token indices a pass stores.  Plain C++17, shared by the kernels and the
// host (tests/cpp/net_layout.cpp compiles it with g++ under the sanitizers, runs the whole chunked
// pipeline with it and compares the records with SNAPReader's).
//
// The record stream is the one `std::istream >> unsigned` yields in the C locale
// (lib/readerwriter.h SNAPReader).  A token is a maximal run of non-whitespace bytes.  A REGULAR
// token is all decimal digits (any length, leading zeros allowed) with value <= 0xFFFFFFFF: it is
// one u32 of the stream.  Any other token is IRREGULAR (`>>` does not treat it as a unit: "4+5" is
// two numbers, "-1" is 4294967295, "12abc" yields 12 and then fails).  The device parses the
// maximal prefix of regular tokens; from the first byte of the first irregular token on, the
// host runs `>>` itself (extraction is stateless at a token boundary).  Token t of the stream
// (device tokens, then the tail's values) is word t of the records: record r = (token 2r,
// token 2r + 1), an odd last value dropped.
//
// A chunk handed to the device starts at a token boundary and ends with a whitespace byte, so no
// token crosses chunks and no parse walks past a chunk.  A lane owns the 16 bytes of one aligned
// word; bytes past the chunk's length in its last word count as whitespace.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SHEEP_HD __host__ __device__
#else
#define SHEEP_HD
#endif

namespace sheep {

constexpr uint32_t NET_WORD = 16;                      // bytes per lane (one 16-byte load)
constexpr uint32_t NET_LANES = 256;                    // lanes (words) per tile
constexpr uint32_t NET_TILE = NET_WORD * NET_LANES;    // bytes per tile
constexpr uint64_t NET_CHUNK_MIN = 4096, NET_CHUNK_MAX = 1ull << 30;  // option net_chunk
constexpr uint64_t NET_NONE = ~0ull;                   // no stop (the stop pair's initial value)

// The device words of one pass (u64 each).
enum { NET_TOTAL = 0,  // tokens of the chunks so far
       NET_BASE,       // NET_TOTAL before the current chunk (its first token's index)
       NET_STOP_TOK,   // smallest index of an irregular token (atomicMin; NET_NONE)
       NET_STOP_OFF,   // its file offset (atomicMin: the token index is monotone in the offset)
       NET_MAX,        // low word: max id + 1 of the stored values (saturating)
       NET_WORDS = 8 };

// The C locale's whitespace: 0x20 and 0x09 .. 0x0D.
SHEEP_HD inline bool net_is_ws(uint32_t b) { return b == 0x20u || b - 9u <= 4u; }
SHEEP_HD inline bool net_is_digit(uint32_t b) { return b - 0x30u <= 9u; }

// Whitespace bits of the four bytes of a little-endian u32 (bit i: byte i).
SHEEP_HD inline uint32_t net_ws4(uint32_t x) {
  return (uint32_t)net_is_ws(x & 0xFFu) | ((uint32_t)net_is_ws((x >> 8) & 0xFFu) << 1) |
         ((uint32_t)net_is_ws((x >> 16) & 0xFFu) << 2) | ((uint32_t)net_is_ws(x >> 24) << 3);
}
// Whitespace mask of a 16-byte word (bit i: byte i) of which `valid` bytes (1 .. 16) belong to the
// chunk; the rest count as whitespace.
SHEEP_HD inline uint32_t net_ws_mask(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3,
                                     uint32_t valid) {
  const uint32_t ws = net_ws4(w0) | (net_ws4(w1) << 4) | (net_ws4(w2) << 8) | (net_ws4(w3) << 12);
  return (ws | (0xFFFFu << valid)) & 0xFFFFu;
}
// Token starts of a word: a non-whitespace byte whose predecessor is whitespace.  pred_ws: the
// byte before the word is whitespace (a chunk's first byte counts as following whitespace).
SHEEP_HD inline uint32_t net_start_mask(uint32_t ws, bool pred_ws) {
  return ~ws & ((ws << 1) | (uint32_t)pred_ws) & 0xFFFFu;
}

// The token that starts at text[pos]: walks to its first whitespace byte, which exists before
// `end` (a chunk ends with whitespace; the bound is a guard, a token that reaches it is
// irregular).  True and *value for a regular token; false for an irregular one.
SHEEP_HD inline bool net_parse_token(const uint8_t* text, uint64_t pos, uint64_t end,
                                     uint32_t* value) {
  uint64_t acc = 0;
  for (; pos < end; ++pos) {
    const uint32_t b = text[pos];
    if (net_is_ws(b)) {
      *value = (uint32_t)acc;
      return true;
    }
    if (!net_is_digit(b)) return false;
    acc = acc * 10u + (b - 0x30u);
    if (acc > 0xFFFFFFFFull) return false;  // (checked per digit: acc never overflows u64)
  }
  return false;
}

// A pass stores the tokens of [lo2, hi2): lo2 = 2 * the range's first record, hi2 = min(2 * its
// end, the first irregular token's index).  Nothing outside is stored, whatever the file holds.
SHEEP_HD inline bool net_in_window(uint64_t t, uint64_t lo2, uint64_t hi2) {
  return t >= lo2 && t < hi2;
}
// max id + 1 of a value, saturating: 0xFFFFFFFF (or 0xFFFFFFFE + 1) is refused by the host.
SHEEP_HD inline uint32_t net_top(uint32_t v) { return v == 0xFFFFFFFFu ? v : v + 1u; }

// Option net_chunk: bytes per chunk, clamped to [4096, 2^30] and rounded down to 16.
inline uint64_t net_chunk_clamp(long long v) {
  uint64_t c = v < (long long)NET_CHUNK_MIN ? NET_CHUNK_MIN : (uint64_t)v;
  if (c > NET_CHUNK_MAX) c = NET_CHUNK_MAX;
  return c & ~15ull;
}
// Where the host cuts a buffer of len bytes that starts at a token boundary: after its last
// whitespace byte.  0: none, the token at its front does not end within one chunk (irregular).
inline uint64_t net_cut(const uint8_t* buf, uint64_t len) {
  while (len && !net_is_ws(buf[len - 1])) --len;
  return len;
}
// The host's chunk loop over two buffers of chunk + 32 bytes each.  read(dst, want) returns the
// bytes it got, fewer than want only at the end of the file; reuse(i) returns once buffer i's
// previous chunk has left it; ship(i, cut, off) hands buf[i][0, cut), whose first byte sits at
// file offset off, to the device.  Every chunk shipped starts at a token boundary and ends with
// whitespace: the rest behind the cut is carried to the front of the next buffer, and the last
// chunk gets one '\n'.  Returns NET_NONE, or the file offset of a token that does not end
// within one chunk (nothing from it on is shipped).
template <class Read, class Reuse, class Ship>
inline uint64_t net_feed(uint8_t* const buf[2], uint64_t chunk, Read read, Reuse reuse, Ship ship) {
  uint64_t carry = 0, carry_at = 0, off = 0;
  bool eof = false;
  for (uint64_t k = 0; !eof; ++k) {
    const int i = (int)(k & 1);
    if (k >= 2) reuse(i);
    if (carry) memcpy(buf[i], buf[i ^ 1] + carry_at, carry);
    const uint64_t want = chunk - carry, got = read(buf[i] + carry, want);
    uint64_t len = carry + got, cut;
    eof = got < want;
    if (eof) {
      buf[i][len++] = '\n';
      cut = len;
    } else if ((cut = net_cut(buf[i], len)) == 0) {
      return off;
    }
    ship(i, cut, off);
    carry = len - cut;
    carry_at = cut;
    off += cut;
  }
  return NET_NONE;
}
// The records [*lo, *hi) of part/num_parts (1-based, graph2tree -l; num_parts 0: all) among R.
inline void net_range(uint64_t R, uint64_t part, uint64_t num_parts, uint64_t* lo, uint64_t* hi) {
  *lo = num_parts ? R * (part - 1) / num_parts : 0;
  *hi = num_parts ? R * part / num_parts : R;
}
inline uint32_t net_tiles(uint64_t n) { return (uint32_t)((n + NET_TILE - 1) / NET_TILE); }

}  // namespace sheep
