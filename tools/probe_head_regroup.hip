// Probe for the graph edits that regrouping a run's head needs (capture_overlap.h, "Regrouping the head"), stand-alone:
//   hipcc --offload-arch=gfx950 -O2 -o probe_head_regroup tools/probe_head_regroup.hip && ./probe_head_regroup
// While a capture is open: a chain of eight small kernels; nodes 1 and 2 rewritten to another kernel (larger grid, 70 KiB of
// dynamic LDS, a 432-byte by-value argument) that does the work of four small ones each; the stream's dependency set walked
// back and nodes 8..3 destroyed; two more kernels captured; instantiate, three replays, results checked.  Every step's error
// code is printed; the first failure ends the program (exit 1), a wrong result exits 2.  The verdict is recorded in
// profiles/head_regroup.json.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#define STEP(call)                                                              \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    printf("%-58s %s (%d)\n", #call, hipGetErrorString(e_), (int)e_);           \
    if (e_ != hipSuccess) return 1;                                             \
  } while (0)

constexpr int kSlots = 16;
constexpr int kBigGrid = 8;
constexpr unsigned kBigLds = 70 * 1024;

__global__ void small_kernel(int* v, int slot) {
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&v[slot], 1);
}
// v[10] := the sum of the eight slots the chain wrote: right only if the kernel runs after all of them
__global__ void sum_kernel(int* v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    int s = 0;
    for (int i = 0; i < 8; ++i) s += v[i];
    v[10] = s;
  }
}
struct BigArg {
  int* v;
  int* blocks_seen;  // [kBigGrid]
  int n;
  int pad;
  int slots[102];
};
static_assert(sizeof(BigArg) == 432, "a by-value argument of a few hundred bytes");
__global__ void big_kernel(BigArg a) {
  extern __shared__ int lds[];
  for (unsigned i = threadIdx.x; i < kBigLds / 4; i += blockDim.x) lds[i] = (int)i;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int last = lds[kBigLds / 4 - 1];  // kBigLds / 4 - 1
    if (last == (int)(kBigLds / 4 - 1)) atomicAdd(&a.blocks_seen[blockIdx.x], 1);
    if (blockIdx.x == gridDim.x - 1)
      for (int i = 0; i < a.n && i < 102; ++i)
        if (a.slots[i] >= 0 && a.slots[i] < kSlots) atomicAdd(&a.v[a.slots[i]], 1);
  }
}

static hipError_t tail_node(hipStream_t s, hipGraphNode_t* node) {
  hipStreamCaptureStatus st;
  unsigned long long id;
  hipGraph_t g;
  const hipGraphNode_t* d = nullptr;
  size_t n = 0;
  hipError_t e = hipStreamGetCaptureInfo_v2(s, &st, &id, &g, &d, &n);
  if (e != hipSuccess) return e;
  if (st != hipStreamCaptureStatusActive || n != 1) return hipErrorInvalidValue;
  *node = d[0];
  return hipSuccess;
}

int main() {
  int *v = nullptr, *seen = nullptr;
  STEP(hipMalloc(&v, kSlots * sizeof(int)));
  STEP(hipMalloc(&seen, 2 * kBigGrid * sizeof(int)));
  STEP(hipMemset(v, 0, kSlots * sizeof(int)));
  STEP(hipMemset(seen, 0, 2 * kBigGrid * sizeof(int)));
  STEP(hipFuncSetAttribute((const void*)big_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBigLds));
  hipStream_t s;
  STEP(hipStreamCreate(&s));
  STEP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  hipGraphNode_t node[8];
  for (int i = 0; i < 8; ++i) {
    hipLaunchKernelGGL(small_kernel, dim3(4), dim3(64), 0, s, v, i);
    STEP(hipGetLastError());
    STEP(tail_node(s, &node[i]));
  }
  // nodes 1 and 2 take over all eight slots
  for (int k = 0; k < 2; ++k) {
    BigArg a;
    memset(&a, 0, sizeof a);
    a.v = v;
    a.blocks_seen = seen + k * kBigGrid;
    a.n = 4;
    for (int i = 0; i < 4; ++i) a.slots[i] = 2 * i + k;
    void* args[1] = {&a};
    hipKernelNodeParams p;
    memset(&p, 0, sizeof p);
    p.func = (void*)big_kernel;
    p.gridDim = dim3(kBigGrid);
    p.blockDim = dim3(256);
    p.sharedMemBytes = kBigLds;
    p.kernelParams = args;
    p.extra = nullptr;
    STEP(hipGraphKernelNodeSetParams(node[k], &p));
  }
  // walk the dependency set back, destroy nodes 8 .. 3
  for (int i = 7; i >= 2; --i) {
    STEP(hipStreamUpdateCaptureDependencies(s, &node[i - 1], 1, hipStreamSetCaptureDependencies));
    STEP(hipGraphDestroyNode(node[i]));
  }
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(64), 0, s, v);
  STEP(hipGetLastError());
  hipLaunchKernelGGL(small_kernel, dim3(4), dim3(64), 0, s, v, 9);
  STEP(hipGetLastError());
  hipGraph_t graph;
  STEP(hipStreamEndCapture(s, &graph));
  size_t nodes = 0;
  STEP(hipGraphGetNodes(graph, nullptr, &nodes));
  printf("nodes in the graph: %zu (expected 4)\n", nodes);
  hipGraphExec_t exec;
  STEP(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
  int hv[kSlots], hs[2 * kBigGrid];
  bool ok = nodes == 4;
  for (int r = 1; r <= 3; ++r) {
    STEP(hipGraphLaunch(exec, s));
    STEP(hipStreamSynchronize(s));
    STEP(hipMemcpy(hv, v, sizeof hv, hipMemcpyDeviceToHost));
    ok = ok && hv[10] == 8 * r;  // the sum kernel saw this replay's eight increments
  }
  STEP(hipMemcpy(hs, seen, sizeof hs, hipMemcpyDeviceToHost));
  for (int i = 0; i < 8; ++i) ok = ok && hv[i] == 3;
  ok = ok && hv[8] == 0 && hv[9] == 3;
  for (int i = 0; i < 2 * kBigGrid; ++i) ok = ok && hs[i] == 3;
  printf("v:");
  for (int i = 0; i < kSlots; ++i) printf(" %d", hv[i]);
  printf("\nblocks_seen:");
  for (int i = 0; i < 2 * kBigGrid; ++i) printf(" %d", hs[i]);
  printf("\nverdict: %s\n", ok ? "accepted, results right" : "WRONG RESULT");
  STEP(hipGraphExecDestroy(exec));
  STEP(hipGraphDestroy(graph));
  STEP(hipStreamDestroy(s));
  STEP(hipFree(v));
  STEP(hipFree(seen));
  return ok ? 0 : 2;
}
