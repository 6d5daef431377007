// The arms of scripts/net_ingest_bench.py in one process on one GPU: an R-MAT graph written once
// as SNAP text and as XS1 records, then, alternating, three runs each of
//   a  SNAPReader into a std::vector + sheep_records_register   (EdgeGraph before the GPU parser)
//   b  sheep_records_load_net                                    (count pass + storing pass)
//   q  the size query + sheep_records_load_net                   (EdgeGraph now: three passes)
//   c  sheep_records_load_dat on the same records
//   d  the staging loop alone: net_feed + uploads, no kernels    (the I/O floor of ONE pass)
// One JSON line per run, then the check that b's records equal a's.
// Usage: net_ingest_bench DIR SCALE [RUNS]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <chrono>
#include <string>
#include <vector>

#include "net_layout.h"
#include "readerwriter.h"
#include "sheep_amd.h"

#define OK(x)                                                                    \
  do {                                                                           \
    if ((x) != 0) {                                                              \
      fprintf(stderr, "%s failed: %s\n", #x, sheep_last_error());                \
      return 1;                                                                  \
    }                                                                            \
  } while (0)

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int staging_only(const char* path, uint64_t chunk, double* sec) {
  using namespace sheep;
  uint8_t* pin[2];
  uint8_t* txt[2];
  hipEvent_t done[2];
  hipStream_t s;
  const double t0 = now();
  OK(hipStreamCreate(&s));
  for (int i = 0; i < 2; ++i) {
    OK(hipHostMalloc((void**)&pin[i], chunk + 32, hipHostMallocDefault));
    OK(hipMalloc((void**)&txt[i], chunk + 32));
    OK(hipEventCreateWithFlags(&done[i], hipEventDisableTiming));
  }
  FILE* f = fopen(path, "rb");
  if (!f) return 1;
  net_feed(
      pin, chunk, [&](uint8_t* dst, uint64_t want) -> uint64_t { return fread(dst, 1, want, f); },
      [&](int i) { (void)hipEventSynchronize(done[i]); },
      [&](int i, uint64_t cut, uint64_t) {
        (void)hipMemcpyAsync(txt[i], pin[i], cut, hipMemcpyHostToDevice, s);
        (void)hipEventRecord(done[i], s);
      });
  OK(hipStreamSynchronize(s));
  fclose(f);
  for (int i = 0; i < 2; ++i) {
    (void)hipHostFree(pin[i]);
    (void)hipFree(txt[i]);
    (void)hipEventDestroy(done[i]);
  }
  (void)hipStreamDestroy(s);
  *sec = now() - t0;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[1];
  const int scale = atoi(argv[2]), runs = argc > 3 ? atoi(argv[3]) : 3;
  const uint64_t m = 16ull << scale;
  const std::string net = dir + "/bench.net", dat = dir + "/bench.dat";
  OK(sheep_gpu_init(0));
  std::vector<uint32_t> uv(2 * m);
  {
    uint32_t* d;
    OK(hipMalloc((void**)&d, 8 * m));
    OK(sheep_rmat_dev(d, scale, 22, 0, m, nullptr));
    OK(hipDeviceSynchronize());
    OK(hipMemcpy(uv.data(), d, 8 * m, hipMemcpyDeviceToHost));
    OK(hipFree(d));
    FILE* f = fopen(net.c_str(), "wb");
    FILE* g = fopen(dat.c_str(), "wb");
    if (!f || !g) return 1;
    std::vector<char> line(1 << 16);
    size_t at = 0;
    for (uint64_t r = 0; r < m; ++r) {
      at += snprintf(line.data() + at, 32, "%u %u\n", uv[2 * r], uv[2 * r + 1]);
      if (at + 32 > line.size()) { fwrite(line.data(), 1, at, f); at = 0; }
      const xs1 rec{uv[2 * r], uv[2 * r + 1], 1.0f};
      fwrite(&rec, sizeof rec, 1, g);
    }
    fwrite(line.data(), 1, at, f);
    printf("{\"records\": %llu, \"text_bytes\": %lld}\n", (unsigned long long)m, (long long)ftello(f));
    fclose(f);
    fclose(g);
  }
  long long chunk = 0;
  OK(sheep_get_option("net_chunk", &chunk));
  std::vector<uint32_t> out(2 * m);
  bool same = true;
  for (int r = 0; r < runs; ++r) {
    double t0 = now();
    {
      std::vector<uint32_t> all;
      SNAPReader rd(net.c_str());
      vid_t X, Y;
      while (rd.read(X, Y)) {
        all.push_back(X);
        all.push_back(Y);
      }
      OK(sheep_records_register(all.data(), all.size() / 2));
      const double t = now() - t0;
      same = same && all == uv;
      OK(sheep_records_release(all.data()));
      printf("{\"arm\": \"a\", \"run\": %d, \"s\": %.4f}\n", r, t);
    }
    uint64_t n = 0;
    uint32_t mx = 0;
    t0 = now();
    OK(sheep_records_load_net(net.c_str(), 0, 0, out.data(), m, &n, &mx));
    printf("{\"arm\": \"b\", \"run\": %d, \"s\": %.4f}\n", r, now() - t0);
    same = same && n == m && out == uv;
    OK(sheep_records_release(out.data()));
    t0 = now();
    OK(sheep_records_load_net(net.c_str(), 0, 0, nullptr, 0, &n, nullptr));
    OK(sheep_records_load_net(net.c_str(), 0, 0, out.data(), n, &n, &mx));
    printf("{\"arm\": \"q\", \"run\": %d, \"s\": %.4f}\n", r, now() - t0);
    OK(sheep_records_release(out.data()));
    t0 = now();
    OK(sheep_records_load_dat(dat.c_str(), 0, 0, out.data(), m, &n, &mx));
    printf("{\"arm\": \"c\", \"run\": %d, \"s\": %.4f}\n", r, now() - t0);
    same = same && n == m && out == uv;
    OK(sheep_records_release(out.data()));
    double d = 0;
    if (staging_only(net.c_str(), (uint64_t)chunk, &d)) return 1;
    printf("{\"arm\": \"d\", \"run\": %d, \"s\": %.4f}\n", r, d);
    fflush(stdout);
  }
  printf("{\"records_equal\": %s}\n", same ? "true" : "false");
  remove(net.c_str());
  remove(dat.c_str());
  return same ? 0 : 1;
}
