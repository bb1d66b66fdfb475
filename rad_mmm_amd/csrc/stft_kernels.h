// Pieces of the STFT -> mel front end shared by stft.hip (one length per call) and collate.hip (ragged batch): the
// scratch layout, the magnitude pass and the zero-padded copy of the mel filterbank.  Both callers must run the very
// same arithmetic: the ragged path is tested bit for bit against the single-length one.
#pragma once
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void pad_cols_kernel(const float* __restrict__ src, int ld_src,
                                                       float* __restrict__ dst, int ld_dst, int rows,
                                                       int cols) {
  const long long total = (long long)rows * ld_dst;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / ld_dst), c = (int)(i - (long long)r * ld_dst);
    dst[i] = c < cols ? src[(long long)r * ld_src + c] : 0.f;
  }
}

__global__ __launch_bounds__(256) void magnitude_kernel(const float* __restrict__ spec, int lds,
                                                        float* __restrict__ mag, int ldm,
                                                        long long rows, int cutoff) {
  const long long total = rows * ldm;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long r = i / ldm;
    const int c = (int)(i - r * ldm);
    float v = 0.f;
    if (c < cutoff) {
      const float re = spec[r * lds + c], im = spec[r * lds + cutoff + c];
      v = sqrtf(re * re + im * im);
    }
    mag[i] = v;
  }
}

inline int grid_for(long long total) {
  long long g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}
inline long long r4(long long x) { return (x + 3) & ~3LL; }

struct StftLayout {
  int F, cutoff, pitch, lds, ldm, ldt;
  long long off_xpad, off_spec, off_mag, off_melb, off_melT, total;
};
inline StftLayout stft_layout(int B, int S, int n_fft, int hop, int n_mel) {
  StftLayout L;
  L.F = 1 + S / hop;
  L.cutoff = n_fft / 2 + 1;
  L.pitch = (int)r4(S + n_fft);
  L.lds = (int)r4(2 * L.cutoff);
  L.ldm = (int)r4(L.cutoff);
  L.ldt = (int)r4(n_mel);
  long long o = 0;
  L.off_xpad = o; o += r4((long long)B * L.pitch);
  L.off_spec = o; o += r4((long long)B * L.F * L.lds);
  L.off_mag = o;  o += r4((long long)B * L.F * L.ldm);
  L.off_melb = o; o += r4((long long)n_mel * L.ldm);
  L.off_melT = o; o += r4((long long)B * L.F * L.ldt);
  L.total = o;
  return L;
}

}  // namespace
