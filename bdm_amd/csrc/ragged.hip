// ragged.hip -- the host plumbing of the packed, ragged batches (ragged.h) and its one kernel.
//   offsets_kernel   the two host offset arrays travel as launch arguments, 32 entries per launch, into the workspace.
#include "ragged.h"

namespace bdm {

constexpr int OFFSETS_PER_LAUNCH = 32;

namespace {

struct OffsetChunk {
  long long a[OFFSETS_PER_LAUNCH], b[OFFSETS_PER_LAUNCH];
};

__global__ void offsets_kernel(OffsetChunk chunk, int first, int count, long long *__restrict__ dev_a, long long *__restrict__ dev_b) {
  const int i = threadIdx.x;
  if (i < count) {  // count <= OFFSETS_PER_LAUNCH, first + count <= b + 1
    dev_a[first + i] = chunk.a[i];
    dev_b[first + i] = chunk.b[i];
  }
}

}  // namespace

int check_first(const char *what, const char *noun, int b, const long long *first, long long *max_count) {
  BDM_REQUIRE(first[0] == 0, "%s: the offsets must start at 0", what);
  *max_count = 0;
  for (int i = 0; i < b; ++i) {
    const long long n = first[i + 1] - first[i];
    BDM_REQUIRE(n >= 0, "%s: offsets decrease at %s %d", what, noun, i);
    if (n > *max_count) *max_count = n;
  }
  return BDM_OK;
}

void send_offsets(int b, const long long *first_a, const long long *first_b, long long *dev_a, long long *dev_b, hipStream_t s) {
  for (int first = 0; first <= b; first += OFFSETS_PER_LAUNCH) {
    OffsetChunk chunk;
    const int count = (b + 1 - first) < OFFSETS_PER_LAUNCH ? (b + 1 - first) : OFFSETS_PER_LAUNCH;
    for (int i = 0; i < OFFSETS_PER_LAUNCH; ++i) {
      chunk.a[i] = i < count ? first_a[first + i] : 0;
      chunk.b[i] = i < count && first_b ? first_b[first + i] : 0;
    }
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, s, chunk, first, count, dev_a, dev_b);
  }
}

int check_overlap(const char *what, const Range *in, int n_in, const Range *out, int n_out) {
  for (int o = 0; o < n_out; ++o) {
    for (int i = 0; i < n_in; ++i)
      BDM_REQUIRE(!ranges_overlap(out[o].p, out[o].bytes, in[i].p, in[i].bytes), "%s: output %d overlaps input %d", what, o, i);
    for (int q = o + 1; q < n_out; ++q)
      BDM_REQUIRE(!ranges_overlap(out[o].p, out[o].bytes, out[q].p, out[q].bytes), "%s: outputs %d and %d overlap", what, o, q);
  }
  return BDM_OK;
}

}  // namespace bdm
