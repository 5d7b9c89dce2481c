// Rate of plain global_store_dwordx4 streams by the shape one wave instruction covers (profiles/store_shapes.txt).
//   hipcc -O3 --offload-arch=gfx950 tools/store_shape_probe.hip -o store_shape_probe
//   store_shape_probe SHAPE WAVES_PER_SIMD MEGABYTES      one configuration per process, one line of output
// A wave writes 8 KB chunks with eight instructions each; the shapes differ only in which 16 bytes a lane takes:
//   a  16 rows x 64 B per instruction: a 16x16 float accumulator, rows 256 B apart (two tiles per chunk)
//   b  16-byte pieces at a 32-byte stride over eight 256-B rows, the next instruction filling the gaps
//   c  four whole 256-B rows per instruction, rows 512 B apart (half the width of a 128-column float matrix)
//   d  one contiguous kilobyte per instruction
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
template <int SHAPE>
__global__ __launch_bounds__(256) void k(float4 *__restrict__ dst, long nchunks) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  const float4 v = make_float4(1.f + lane, 2.f, 3.f, 4.f + blockIdx.x);
  for (long c = wave; c < nchunks; c += nwaves) {
    float4 *o = dst + c * 512;  // 8 KB = 512 pieces
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      int piece;
      if (SHAPE == 0) piece = (t >> 2) * 256 + (lane & 15) * 16 + (t & 3) * 4 + (lane >> 4);
      else if (SHAPE == 1) piece = (t >> 1) * 128 + (lane >> 3) * 16 + (lane & 7) * 2 + (t & 1);
      else if (SHAPE == 2) piece = ((t & 3) * 4 + (lane >> 4)) * 32 + (t >> 2) * 16 + (lane & 15);
      else piece = t * 64 + lane;
      o[piece] = v;
    }
  }
}
int main(int argc, char **argv) {
  if (argc != 4) return fprintf(stderr, "usage: %s a|b|c|d waves_per_simd megabytes\n", argv[0]), 2;
  const int shape = argv[1][0] - 'a', wps = atoi(argv[2]);
  const long nchunks = atol(argv[3]) * 1000000L / 8192;
  if (shape < 0 || shape > 3 || wps < 1 || wps > 8 || nchunks < 1) return 2;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
  float4 *d;
  if (hipMalloc(&d, nchunks * 8192) != hipSuccess || hipMemset(d, 0, nchunks * 8192) != hipSuccess) return 1;
  const unsigned grid = prop.multiProcessorCount * wps;  // 256 threads = one wave per SIMD
  auto go = [&] {
    if (shape == 0) k<0><<<grid, 256>>>(d, nchunks);
    else if (shape == 1) k<1><<<grid, 256>>>(d, nchunks);
    else if (shape == 2) k<2><<<grid, 256>>>(d, nchunks);
    else k<3><<<grid, 256>>>(d, nchunks);
  };
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return 1;
  go(); go();
  float best = 1e30f, sum = 0;
  const int reps = 10;
  for (int r = 0; r < reps; ++r) {
    float ms;
    (void)hipEventRecord(e0); go(); (void)hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return 1;
    best = ms < best ? ms : best; sum += ms;
  }
  // every piece written exactly once: the first and last chunk hold lane-tagged values everywhere
  float4 h[1024];
  if (hipMemcpy(h, d, 8192, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(h + 512, d + (nchunks - 1) * 512, 8192, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  int bad = 0;
  for (int i = 0; i < 1024; ++i) bad += !(h[i].x >= 1.f && h[i].x <= 64.f && h[i].y == 2.f);
  const double gb = nchunks * 8192 / 1e9;
  printf("shape %c  %d waves/SIMD  %.3f GB  mean %.3f ms  best %.3f ms  %.2f TB/s (mean)  %.2f TB/s (best)  bad=%d\n", argv[1][0], wps, gb,
         sum / reps, best, gb / (sum / reps), gb / best, bad);
  return bad != 0;
}
