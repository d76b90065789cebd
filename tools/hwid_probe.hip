// hwid_probe.hip -- where the hardware puts the waves of the fused pack kernel's workgroups.
// A grid of 4 x CU-count workgroups of 256 threads, launched with the pack kernel's footprint (launch bounds 256 x 4, 120 VGPRs, its LDS), so that
// four of them are resident on every CU as the pack kernel's are.  Every wave reads HW_REG_HW_ID and HW_REG_XCC_ID and writes one row
//   block wave xcc se sh cu simd slot
// through an ordinary vector store; a workgroup stays for ~50 us (a bounded wait on the clock), so the whole grid is resident at once.
// The summary answers: does wave k of a workgroup run on SIMD k?  Which block indices share a CU -- does a function of blockIdx tell them apart?
//   hipcc --offload-arch=gfx950 -O2 -o tools/hwid_probe tools/hwid_probe.hip && tools/hwid_probe [lds_bytes] > profiles/<tag>_placement.txt
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(256, 4) void probe_kernel(uint32_t* __restrict__ out, uint32_t spin_ticks) {
    extern __shared__ uint8_t smem[];
    asm volatile("v_mov_b32 v119, 0" ::: "v119");                // the kernel allocates 120 VGPRs, as the pack kernel does
    smem[threadIdx.x] = (uint8_t)threadIdx.x;
    const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);       // HW_REG_HW_ID, all 32 bits
    const uint32_t xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);     // HW_REG_XCC_ID
    const uint64_t t0 = wall_clock64();
    for (int i = 0; i < 100000 && wall_clock64() - t0 < spin_ticks; ++i) __builtin_amdgcn_s_sleep(8);      // (bounded: ends by the count if the clock stood still)
    if ((threadIdx.x & 63u) == 0) {
        uint32_t* o = out + 2 * (blockIdx.x * 4 + (threadIdx.x >> 6));
        o[0] = hw; o[1] = xcc;
    }
}

int main(int argc, char** argv) {
    const size_t lds = argc > 1 ? (size_t)atol(argv[1]) : 36 * 1024;
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount, blocks = 4 * cus;
    uint32_t* d;
    CHECK(hipMalloc(&d, (size_t)blocks * 4 * 2 * sizeof(uint32_t)));
    CHECK(hipMemset(d, 0xFF, (size_t)blocks * 4 * 2 * sizeof(uint32_t)));
    CHECK(hipFuncSetAttribute((const void*)probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    probe_kernel<<<blocks, 256, lds>>>(d, 5000);                 // 5 000 ticks of the 100 MHz clock = 50 us
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<uint32_t> h((size_t)blocks * 8);
    CHECK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost));
    printf("# %s, %d CUs, %d workgroups of 256 threads, %zu B of LDS each\n# block wave xcc se sh cu simd slot\n", prop.name, cus, blocks, lds);
    int wave_is_simd = 0, waves = 0;
    std::map<uint32_t, std::vector<int>> by_cu;                  // (xcc, se, sh, cu) -> blocks
    for (int b = 0; b < blocks; ++b)
        for (int w = 0; w < 4; ++w) {
            const uint32_t hw = h[2 * (b * 4 + w)], xcc = h[2 * (b * 4 + w) + 1] & 15u;
            const uint32_t slot = hw & 15u, simd = (hw >> 4) & 3u, cu = (hw >> 8) & 15u, sh = (hw >> 12) & 1u, se = (hw >> 13) & 7u;
            printf("%d %d %u %u %u %u %u %u\n", b, w, xcc, se, sh, cu, simd, slot);
            ++waves; if (simd == (uint32_t)w) ++wave_is_simd;
            if (w == 0) by_cu[(xcc << 12) | (se << 8) | (sh << 4) | cu].push_back(b);
        }
    printf("# waves with simd == wave index: %d of %d\n", wave_is_simd, waves);
    int full = 0, mod4 = 0, div_cu = 0, div_cu_xcc = 0;
    for (auto& kv : by_cu) {
        const std::vector<int>& v = kv.second;
        if (v.size() != 4) continue;
        ++full;
        unsigned a = 0, c = 0, e = 0;
        for (int b : v) { a |= 1u << (b & 3); c |= 1u << ((b / cus) & 3); e |= 1u << ((b / 8) & 3); }
        mod4 += a == 15u; div_cu += c == 15u; div_cu_xcc += e == 15u;
    }
    printf("# CUs seen: %zu, with exactly four workgroups: %d\n", by_cu.size(), full);
    printf("# of those, the four are told apart by  block %% 4: %d   (block / CUs) %% 4: %d   (block / 8) %% 4: %d\n", mod4, div_cu, div_cu_xcc);
    for (auto& kv : by_cu) {
        printf("# xcc %u se %u sh %u cu %2u:", kv.first >> 12, (kv.first >> 8) & 15u, (kv.first >> 4) & 15u, kv.first & 15u);
        for (int b : kv.second) printf(" %d", b);
        printf("\n");
    }
    CHECK(hipFree(d));
    return 0;
}
