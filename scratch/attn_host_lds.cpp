// Dynamic LDS bytes of every attention launch of a build of libvog_hip.so, without a GPU (attn_plan: the kernel trace reports
// static LDS only, so the parent's byte counts are taken here). The program defines the HIP calls the attention launchers
// make (and the two behind <<< >>>); the executable's definitions come first in symbol lookup, so the library's launches land
// here and are printed, not run.
//
//   g++ -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -rdynamic scratch/attn_host_lds.cpp -ldl -o scratch/attn_host_lds
//   scratch/attn_host_lds LIB.so < ROWS.txt      (ROWS.txt: scratch/attn_launch_rows.py --rows)
//
// A row is "rel dp N guard precleared split out_lo" or "struct dp nppf nsrl q_visual guard split out_lo" (S = 2, H = 1, as the
// table of attn_launch_rows.py); a line out is "rc n  grid block lds ..." with one triple per launch.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "vog_hip.h"

struct Rec { unsigned grid, block; size_t lds; };
static std::vector<Rec> g_recs;

extern "C" hipError_t hipLaunchKernel(const void*, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
  g_recs.push_back({grid.x, block.x, lds});
  return hipSuccess;
}
// (the <<< >>> of a launch: the configuration is pushed, the kernel's host stub pops it and calls hipLaunchKernel)
static dim3 g_grid, g_block;
static size_t g_lds;
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t) {
  g_grid = grid; g_block = block; g_lds = lds;
  return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* st) {
  *grid = g_grid; *block = g_block; *lds = g_lds; *st = nullptr;
  return hipSuccess;
}
extern "C" hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }

int main(int argc, char** argv) {
  void* h = dlopen(argv[1], RTLD_NOW | RTLD_GLOBAL);
  if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
  auto rel = (int (*)(const vog_attn_args*, void*))dlsym(h, "vog_rel_attention_fwd");
  auto st = (int (*)(const vog_attn_struct_args*, void*))dlsym(h, "vog_rel_attention_struct_fwd");
  static char fake[64];
  void* const P = fake;            // never dereferenced: nothing is launched
  char e[16];
  int v[7];
  auto pad = [](int n) { return (n + 31) / 32 * 32; };
  while (scanf("%15s", e) == 1) {
    g_recs.clear();
    int rc;
    if (!strcmp(e, "rel")) {
      for (int i = 0; i < 6; ++i) if (scanf("%d", &v[i]) != 1) return 3;
      vog_attn_args a{};
      a.q = a.k = a.vt = P; a.out16 = P;
      a.S = 2; a.H = 1; a.dp = v[0]; a.N = v[1]; a.npad = pad(v[1]); a.n_box = a.NP = v[1]; a.seq_per_vid = 1;
      a.inv_scale = 0.125f; a.dtype = VOG_BF16;
      if (v[2]) a.guard_flag = (int*)P;
      a.guard_precleared = v[3];
      if (v[4]) a.q_lo = a.k_lo = P;
      if (v[5]) a.out16_lo = P;
      rc = rel(&a, nullptr);
    } else {
      for (int i = 0; i < 7; ++i) if (scanf("%d", &v[i]) != 1) return 3;
      vog_attn_struct_args a{};
      a.q = a.kv = a.vv = P; a.pl = (const float*)P; a.out16 = P;
      a.S = 2; a.H = 1; a.dp = v[0]; a.nppf = v[1]; a.nsrl = v[2]; a.q_visual = v[3];
      a.npad_q = pad(v[2] * v[1]); a.npad_kv = pad(v[1]); a.nfrm = 2; a.lang_per_vid = 0; a.nc_v = 1; a.seq_per_vid = 2; a.NP = 2 * v[1];
      a.inv_scale = 0.125f; a.dtype = VOG_BF16;
      if (v[4]) a.guard_flag = (int*)P;
      if (v[5]) a.q_lo = a.kv_lo = P;
      if (v[6]) a.out16_lo = P;
      rc = st(&a, nullptr);
    }
    printf("%d %zu", rc, g_recs.size());
    for (const Rec& r : g_recs) printf("  %u %u %zu", r.grid, r.block, r.lds);
    printf("\n");
  }
  return 0;
}
