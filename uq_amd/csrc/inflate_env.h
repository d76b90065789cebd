// inflate_env.h -- what the environments of the two inflate paths (inflate.hip: BGZF members, inflate_stream.hip: gzip in chunks) have in
// common around the decoders of inflate_core.h / inflate_stream.h: where the compressed bytes come from on the device and on the host, and
// the CRC-32 plumbing.  Off is the type of a byte offset: uint32_t for a member, uint64_t for a whole file.
#pragma once
#include "common.h"
#include "inflate_core.h"

struct X2n { uint32_t v[32]; };              // x^(2^k) mod the CRC polynomial, passed by value (kernel arguments: scalar loads)

// The wave-uniform source of a decoder: the compressed bytes 256 at a time, one dword per lane (a coalesced load), words handed to the bit
// reader with v_readlane
template <class Off>
struct DevSrc {
    const uint8_t* p;
    Off len, wbase;
    uint32_t mine, lane;
    __device__ void load(Off base) {
        wbase = base;
        const Off b = base + 4 * lane;
        uint32_t v = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (b + k < len) v |= (uint32_t)p[b + k] << (8 * k);
        mine = v;
    }
    __device__ uint32_t word(Off off) {
        // wave-uniform by construction; this tells the compiler (the builtin returns a signed int: the low half must not sign-extend)
        const uint32_t lo32 = __builtin_amdgcn_readfirstlane((uint32_t)off);
        if constexpr (sizeof(Off) == 8) off = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(off >> 32)) << 32 | lo32;
        else off = lo32;
        if (off < wbase || off + 4 > wbase + 256) load(off & ~(Off)3);
        const uint32_t rel = (uint32_t)(off - wbase), i = rel >> 2, s = (rel & 3) * 8;
        const uint32_t lo = __builtin_amdgcn_readlane(mine, i);
        if (!s) return lo;
        const uint32_t hi = __builtin_amdgcn_readlane(mine, (i + 1) & 63);
        return (lo >> s) | (hi << (32 - s));
    }
    __device__ uint32_t byte(Off o) const { return o < len ? p[o] : 0u; }              // per lane (stored blocks)
};

// Plain byte pointers: the host's source, and on the device the finder's (every lane reads its own offsets)
template <class Off>
struct HostSrc {
    const uint8_t* p;
    Off len;
    __host__ __device__ uint32_t word(Off off) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if ((uint64_t)off + k < len) v |= (uint32_t)p[off + k] << (8 * k);
        return v;
    }
    __host__ __device__ uint32_t byte(Off o) const { return o < len ? p[o] : 0u; }
};

// The host's CRC-32 byte table
inline const uint32_t* crc_table() {
    struct Table {
        uint32_t t[256];
        Table() { for (uint32_t e = 0; e < 256; ++e) t[e] = uq_crc_table_entry(e); }
    };
    static const Table tab;
    return tab.t;
}

// A message's crc0 by the lanes of a wave: each lane's segment p[0, n) (p 4-byte aligned) continues its c, is carried over the `after` bytes
// of the message behind it with the shift operator, and the lanes' values are XOR-ed.  Every lane returns the whole message's crc0.
__device__ __forceinline__ uint32_t wave_crc0(const uint32_t* table, const X2n& x2n, uint32_t c, const uint8_t* p, uint32_t n, uint64_t after) {
    uint32_t i = 0;
    for (; i + 4 <= n; i += 4) {
        c ^= *(const uint32_t*)(p + i);
        c = table[c & 0xFF] ^ (c >> 8);
        c = table[c & 0xFF] ^ (c >> 8);
        c = table[c & 0xFF] ^ (c >> 8);
        c = table[c & 0xFF] ^ (c >> 8);
    }
    c = uq_crc0_bytes(table, c, p + i, n - i);
    c = uq_crc_multmodp(uq_crc_shift_op(x2n.v, after), c);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c ^= __shfl_xor(c, d, 64);
    return c;
}
