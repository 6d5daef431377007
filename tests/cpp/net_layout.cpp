// The .net ingest's arithmetic (sheep_amd/csrc/net_layout.h) run as the whole chunked pipeline on
// the host: the chunk loop with its carry and final '\n' (net_feed itself), and per chunk what the
// three kernels of sheep_ingest.hip do with the header's functions: every lane's 16-byte word,
// its whitespace and token-start masks (the predecessor from the neighbouring lane, or one byte
// load at a wave's first lane), the tile counts, their scan onto the running token base, each
// start's rank, the one-token parse, the window guard, the stop pair; then the host tail.  The
// record stream must equal SNAPReader's (sheep_amd/lib/readerwriter.h) on the same bytes in a
// temporary file, for the whole file and for -l parts, at chunk sizes 16, 32, 48 and 4096.
// Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_net_layout.py.  Usage: net_layout TMPFILE.  Prints "ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "net_layout.h"
#include "readerwriter.h"

using namespace sheep;

static int fails = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++fails <= 40) {                             \
        fprintf(stderr, "FAIL %s: ", #c);              \
        fprintf(stderr, __VA_ARGS__);                  \
        fprintf(stderr, "\n");                         \
      }                                                \
    }                                                  \
  } while (0)

// ---- the device side of one chunk, lane by lane ------------------------------------------------

// net_lane_starts of sheep_ingest.hip.  prev_ws: the whitespace mask of word w - 1 (what the
// neighbouring lane holds); a wave's first lane classifies the byte before its word instead.
static uint32_t lane_starts(const uint8_t* text, uint32_t n, uint32_t w, uint32_t* ws_out) {
  const uint32_t nwords = (n + NET_WORD - 1) / NET_WORD;
  uint32_t ws = 0xFFFFu;
  if (w < nwords) {
    uint32_t x[4];
    memcpy(x, text + (size_t)w * NET_WORD, 16);  // the lane's 16-byte load (little-endian words)
    ws = net_ws_mask(x[0], x[1], x[2], x[3], std::min(NET_WORD, n - w * NET_WORD));
  }
  uint32_t pred = (*ws_out >> 15) & 1u;  // the lane below's mask, before it is replaced
  if ((w & 63u) == 0) pred = (w == 0 || w >= nwords) ? 1u : net_is_ws(text[w * NET_WORD - 1]);
  *ws_out = ws;
  return net_start_mask(ws, pred != 0);
}

struct Device {
  uint64_t state[NET_WORDS];
  std::vector<uint32_t> uv;  // the caller's records buffer, cap records; never indexed past it
  Device() {
    memset(state, 0, sizeof state);
    state[NET_STOP_TOK] = state[NET_STOP_OFF] = NET_NONE;
  }
  // launch_net_chunk: text holds n bytes; its allocation runs to the next multiple of 16.
  void chunk(const uint8_t* text, uint32_t n, uint64_t file_off, bool store, uint64_t lo2,
             uint64_t hi2) {
    const uint32_t nt = net_tiles(n);
    std::vector<uint32_t> tiles(nt);
    for (uint32_t b = 0; b < nt; ++b) {  // k_net_count
      uint32_t c = 0, ws = 0;
      for (uint32_t l = 0; l < NET_LANES; ++l)
        c += __builtin_popcount(lane_starts(text, n, b * NET_LANES + l, &ws));
      tiles[b] = c;
    }
    uint32_t run = 0;  // k_net_scan
    for (uint32_t b = 0; b < nt; ++b) {
      const uint32_t v = tiles[b];
      tiles[b] = run;
      run += v;
    }
    state[NET_BASE] = state[NET_TOTAL];
    state[NET_TOTAL] += run;
    for (uint32_t b = 0; b < nt; ++b) {  // k_net_parse
      uint32_t excl = 0, ws = 0;
      for (uint32_t l = 0; l < NET_LANES; ++l) {
        const uint32_t w = b * NET_LANES + l;
        uint32_t starts = lane_starts(text, n, w, &ws);
        uint64_t t = state[NET_BASE] + tiles[b] + excl;
        excl += __builtin_popcount(starts);
        for (; starts; starts &= starts - 1, ++t) {
          if (store && !net_in_window(t, lo2, hi2)) continue;
          const uint32_t pos = w * NET_WORD + (uint32_t)__builtin_ctz(starts);
          uint32_t v;
          if (net_parse_token(text, pos, n, &v)) {
            if (store) {
              uv.at(t - lo2) = v;
              state[NET_MAX] = std::max<uint64_t>(state[NET_MAX], net_top(v));
            }
          } else if (!store) {
            state[NET_STOP_TOK] = std::min<uint64_t>(state[NET_STOP_TOK], t);
            state[NET_STOP_OFF] = std::min<uint64_t>(state[NET_STOP_OFF], file_off + pos);
          }
        }
      }
    }
  }
};

// net_pass of sheep_capi.cpp: net_feed over two buffers; every "upload" is a copy into a device
// buffer of exactly the chunk's bytes rounded up to 16 (the rest poisoned with digits, and the
// sanitizer sees any read past it).
static uint64_t pass(const std::string& file, uint64_t chunk, Device& D, bool store, uint64_t lo2,
                     uint64_t hi2) {
  std::vector<uint8_t> b0(chunk + 32, '7'), b1(chunk + 32, '7');
  uint8_t* buf[2] = {b0.data(), b1.data()};
  size_t at = 0;
  uint64_t shipped_end = 0;
  return net_feed(
      buf, chunk,
      [&](uint8_t* dst, uint64_t want) -> uint64_t {
        const uint64_t got = std::min<uint64_t>(want, file.size() - at);
        memcpy(dst, file.data() + at, got);
        at += got;
        return got;
      },
      [&](int) {},
      [&](int i, uint64_t cut, uint64_t off) {
        CHECK(cut >= 1 && cut <= chunk + 1, "cut %llu", (unsigned long long)cut);
        CHECK(net_is_ws(buf[i][cut - 1]), "chunk at %llu does not end with whitespace",
              (unsigned long long)off);
        CHECK(off == shipped_end, "chunks not contiguous");
        CHECK(off == 0 || net_is_ws((uint8_t)file[off - 1]), "chunk starts inside a token");
        shipped_end = off + cut;
        std::vector<uint8_t> dev((cut + 15) / 16 * 16, '7');
        memcpy(dev.data(), buf[i], cut);
        D.chunk(dev.data(), (uint32_t)cut, off, store, lo2, hi2);
      });
}

struct Stream {
  std::vector<uint32_t> uv;  // 2 m values
  uint32_t mx = 0;
};

// net_plan + net_store of sheep_capi.cpp.
static Stream ingest(const std::string& file, uint64_t chunk, uint64_t part, uint64_t num_parts) {
  Device C;
  const uint64_t long_token = pass(file, chunk, C, false, 0, 0);
  const uint64_t t_dev = std::min(C.state[NET_TOTAL], C.state[NET_STOP_TOK]);
  const uint64_t tail_at = C.state[NET_STOP_TOK] != NET_NONE ? C.state[NET_STOP_OFF] : long_token;
  std::vector<uint32_t> tail;
  if (tail_at != NET_NONE) {
    CHECK(tail_at < file.size(), "tail offset %llu", (unsigned long long)tail_at);
    std::istringstream in(file.substr(tail_at));
    unsigned v;
    while (in >> v) tail.push_back(v);
  }
  uint64_t lo, hi;
  net_range((t_dev + tail.size()) / 2, part, num_parts, &lo, &hi);
  const uint64_t lo2 = 2 * lo, hi2 = 2 * hi;
  Stream S;
  Device D;
  D.uv.assign(2 * (hi - lo), 0xDEADBEEFu);
  if (std::min(hi2, t_dev) > lo2) pass(file, chunk, D, true, lo2, std::min(hi2, t_dev));
  S.mx = (uint32_t)D.state[NET_MAX];
  const uint64_t a = std::max(lo2, t_dev);
  for (uint64_t t = a; t < hi2; ++t) {
    D.uv.at(t - lo2) = tail.at(t - t_dev);
    S.mx = std::max(S.mx, net_top(tail[t - t_dev]));
  }
  S.uv = D.uv;
  return S;
}

// ---- the reference: SNAPReader on the same bytes ----------------------------------------------

static const char* g_tmp;

static std::vector<uint32_t> snap(const std::string& file) {
  FILE* f = fopen(g_tmp, "wb");
  if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) {
    fprintf(stderr, "cannot write %s\n", g_tmp);
    exit(2);
  }
  fclose(f);
  std::vector<uint32_t> uv;
  SNAPReader rd(g_tmp);
  vid_t X, Y;
  while (rd.read(X, Y)) {
    uv.push_back(X);
    uv.push_back(Y);
  }
  return uv;
}

static std::string show(const std::string& s) {
  std::string o;
  for (unsigned char ch : s.substr(0, 60)) {
    char b[8];
    if (ch >= 0x21 && ch < 0x7F) o += (char)ch;
    else { snprintf(b, sizeof b, "\\x%02x", ch); o += b; }
  }
  return o;
}

static const uint64_t kChunks[] = {16, 32, 48, 4096};

static void check_text(const std::string& file, const std::vector<uint32_t>* listed) {
  const std::vector<uint32_t> want = snap(file);
  if (listed) CHECK(want == *listed, "SNAPReader differs from the case table on '%s'", show(file).c_str());
  const uint64_t R = want.size() / 2;
  for (uint64_t chunk : kChunks) {
    for (uint64_t part = 0; part <= 3; ++part) {
      const Stream S = ingest(file, chunk, part, part ? 3 : 0);
      uint64_t lo, hi;
      net_range(R, part, part ? 3 : 0, &lo, &hi);
      const std::vector<uint32_t> w(want.begin() + 2 * lo, want.begin() + 2 * hi);
      uint32_t mx = 0;
      for (uint32_t v : w) mx = std::max(mx, net_top(v));
      CHECK(S.uv == w, "records differ: '%s' chunk %llu part %llu (%zu vs %zu values)",
            show(file).c_str(), (unsigned long long)chunk, (unsigned long long)part, S.uv.size(),
            w.size());
      CHECK(S.mx == mx, "max id: '%s' chunk %llu part %llu: %u vs %u", show(file).c_str(),
            (unsigned long long)chunk, (unsigned long long)part, S.mx, mx);
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  g_tmp = argv[1];
  const uint32_t M = 4294967295u;
  struct Case {
    std::string text;
    std::vector<uint32_t> uv;
  };
  const std::vector<Case> cases = {
      {"1 2\n3 4\n", {1, 2, 3, 4}},
      {"1 2 3", {1, 2}},
      {"1 2\n# c\n3 4\n", {1, 2}},
      {"# h\n1 2\n", {}},
      {"+5 6 7 8", {5, 6, 7, 8}},
      {"1 -0 3 4", {1, 0, 3, 4}},
      {"007 0008 1 2", {7, 8, 1, 2}},
      {"12abc 3 4 5", {}},
      {"1 12abc 3 4", {1, 12}},
      {"4294967295 1 2 3", {M, 1, 2, 3}},
      {"4294967296 1 2 3", {}},
      {"1 99999999999999999999999 2 3", {}},
      {"1\r\n2\r\n\v3\f4", {1, 2, 3, 4}},
      {"1 2 0x10 3", {1, 2}},
      {"1 2 3 4.", {1, 2, 3, 4}},
      {"1 2 - 3 4 5", {1, 2}},
      {"1 2 3 " + std::string(31, '0') + "4 5 6", {1, 2, 3, 4, 5, 6}},
      {"1 2 3 4+5 6", {1, 2, 3, 4, 5, 6}},
      {"1 2 3 4-5 6 7", {1, 2, 3, 4, 4294967291u, 6}},
      {"-1 2 3 4", {M, 2, 3, 4}},
      {std::string("1 2 3\0 4 5 6", 12), {1, 2}},
  };
  for (const Case& c : cases) check_text(c.text, &c.uv);
  // the empty file; whitespace only; one token; no trailing newline; a token of 5000 zeros
  for (const std::string& t : {std::string(), std::string(" \t\n\v\f\r  "), std::string("17"),
                               std::string("5 6\n7 8"), std::string(40, ' ') + "3 4",
                               "1 " + std::string(5000, '0') + "2 3 4\n"})
    check_text(t, nullptr);
  // every byte class against the C locale's isspace / isdigit
  for (uint32_t b = 0; b < 256; ++b) {
    CHECK(net_is_ws(b) == (b == ' ' || (b >= '\t' && b <= '\r')), "ws class of %u", b);
    CHECK(net_is_digit(b) == (b >= '0' && b <= '9'), "digit class of %u", b);
  }
  CHECK(net_chunk_clamp(1) == 4096 && net_chunk_clamp(-5) == 4096 && net_chunk_clamp(4111) == 4096 &&
            net_chunk_clamp(1ll << 40) == (1ull << 30) && net_chunk_clamp(32 << 20) == (32u << 20),
        "net_chunk_clamp");
  // 200 seeded random texts of at most 2 KB
  std::mt19937_64 rng(20240611);
  const char wsb[6] = {' ', '\t', '\n', '\v', '\f', '\r'};
  const char odd[] = {'#', '-', '+', '.', 'a', 'x', '\0', '%', ',', (char)0xC3};
  for (int it = 0; it < 200; ++it) {
    std::string t;
    const size_t target = 1 + rng() % 2000;
    if (rng() % 3 == 0) t.append(rng() % 4, wsb[rng() % 6]);
    while (t.size() < target) {
      uint64_t v;
      switch (rng() % 8) {
        case 0: v = 4294967295ull - rng() % 3; break;            // just below 2^32
        case 1: v = rng() % 40 ? rng() % 100 : 4294967296ull + rng() % 3; break;  // rarely above
        case 2: v = rng() % 10; break;
        default: v = rng() >> (32 + rng() % 32); break;          // 0 .. 32 bits
      }
      if (rng() % 6 == 0) t.append(1 + rng() % (rng() % 9 ? 4 : 40), '0');  // leading zeros
      t += std::to_string(v);
      size_t run = 1 + (rng() % 4 == 0 ? rng() % 20 : rng() % 2);  // runs of separators
      while (run--) t += wsb[rng() % 6];
    }
    if (rng() % 2) while (!t.empty() && net_is_ws((uint8_t)t.back())) t.pop_back();
    if (it % 5 == 0 && !t.empty()) t[rng() % t.size()] = odd[rng() % sizeof odd];
    if (t.size() > 2048) t.resize(2048);
    check_text(t, nullptr);
  }
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
