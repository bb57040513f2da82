// Copy the first n_rows cached rows of every (layer, kv head) of a K and a V cache from one
// source to up to 7 destinations in one launch (kernels.h KvCopyArgs; include/llmi.h has the
// contract of llmi_kv_copy_rows): what a fork of a batch slot does to the cache.
//
// The layout is the engine's, [layers, kv_heads, max_seq, 128]: the copied part of a (layer,
// head) segment is one contiguous run of n_rows * row_bytes bytes (a multiple of 128) that starts
// on a 16-byte boundary, and the segments lie max_seq * row_bytes apart. A work item is one
// 16 KiB chunk of one segment: every lane issues its four 16-byte loads before the first store,
// then stores each vector once per destination from the registers, so a source byte is read once
// however many destinations there are. The KV8 scales [layers, kv_heads, max_seq] fp16 are one
// more item per segment: their runs are n_rows * 2 bytes at max_seq * 2 byte strides, so a run
// starts on a 2-byte boundary only -- single halves up to the first 16-byte boundary, 16-byte
// vectors, single halves for the rest (source and destinations share the misalignment: their
// bases are 16-byte aligned). Nothing at or after row n_rows is written. The grid is sized from
// the CU count and strides over the items; no LDS, no atomics.
#include "kernels.h"

namespace llmi {
namespace {

constexpr int kCopyT = 256;
constexpr int kCopyVecs = 4;                         // 16-byte loads in flight per lane
constexpr size_t kCopyChunk = (size_t)kCopyT * kCopyVecs * 16;  // bytes of one work item
constexpr int kCopyWgPerCu = 8;                      // 128 KiB of loads in flight per CU

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct KvCopyKernelArgs {
    const char* src[2];             // K, V
    const unsigned short* src_s[2]; // their scales (null: none)
    char* dst[2][kKvCopyMaxDst];
    unsigned short* dst_s[2][kKvCopyMaxDst];
    int n_dst;
    int segs;               // layers * kv_heads
    size_t seg_stride;      // bytes between two segments' starts
    size_t seg_bytes;       // bytes copied of each
    int chunks;             // work items per segment
    size_t sc_stride;       // scales: halves between two segments' starts
    size_t sc_n;            // ... and halves copied of each
};

// the store of one value to every destination (constant indices: the pointers stay kernel arguments)
#define LLMI_FOR_DST(n, body)                  \
    _Pragma("unroll") for (int d_ = 0; d_ < kKvCopyMaxDst; ++d_) { \
        if (d_ < (n)) { body; }                \
    }

__global__ __launch_bounds__(kCopyT) void kv_copy_rows_kernel(KvCopyKernelArgs a) {
    const size_t data_items = (size_t)2 * a.segs * a.chunks;
    const size_t items = data_items + (a.src_s[0] ? (size_t)2 * a.segs : 0);
    const int t = threadIdx.x;
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        if (it < data_items) {
            const int chunk = (int)(it % a.chunks);
            const size_t sg = it / a.chunks;  // [which][segment]
            const int which = sg >= (size_t)a.segs;
            const size_t seg = sg - (which ? a.segs : 0);
            const size_t base = seg * a.seg_stride;
            const size_t off0 = (size_t)chunk * kCopyChunk + (size_t)t * 16;
            const char* s = (which ? a.src[1] : a.src[0]) + base;
            u32x4 v[kCopyVecs];
#pragma unroll
            for (int i = 0; i < kCopyVecs; ++i) {
                const size_t off = off0 + (size_t)i * kCopyT * 16;
                if (off < a.seg_bytes) v[i] = *reinterpret_cast<const u32x4*>(s + off);
            }
#pragma unroll
            for (int i = 0; i < kCopyVecs; ++i) {
                const size_t off = off0 + (size_t)i * kCopyT * 16;
                if (off < a.seg_bytes) {
                    LLMI_FOR_DST(a.n_dst,
                                 *reinterpret_cast<u32x4*>((which ? a.dst[1][d_] : a.dst[0][d_]) + base + off) = v[i])
                }
            }
        } else {
            const size_t sg = it - data_items;
            const int which = sg >= (size_t)a.segs;
            const size_t base = (sg - (which ? a.segs : 0)) * a.sc_stride;  // in halves
            const unsigned short* s = (which ? a.src_s[1] : a.src_s[0]) + base;
            // halves up to the first 16-byte boundary, whole vectors, the rest
            const size_t mis = (reinterpret_cast<size_t>(s) & 15) / 2;
            const size_t head = mis ? (8 - mis < a.sc_n ? 8 - mis : a.sc_n) : 0;
            const size_t vecs = (a.sc_n - head) / 8;
            const size_t tail0 = head + vecs * 8;
            for (size_t i = t; i < head; i += kCopyT) {
                const unsigned short h = s[i];
                LLMI_FOR_DST(a.n_dst, (which ? a.dst_s[1][d_] : a.dst_s[0][d_])[base + i] = h)
            }
            for (size_t q = t; q < vecs; q += kCopyT) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(s + head + q * 8);
                const size_t o = base + head + q * 8;
                LLMI_FOR_DST(a.n_dst, *reinterpret_cast<u32x4*>((which ? a.dst_s[1][d_] : a.dst_s[0][d_]) + o) = v)
            }
            for (size_t i = tail0 + t; i < a.sc_n; i += kCopyT) {
                const unsigned short h = s[i];
                LLMI_FOR_DST(a.n_dst, (which ? a.dst_s[1][d_] : a.dst_s[0][d_])[base + i] = h)
            }
        }
    }
}
#undef LLMI_FOR_DST

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// LLMI_EINVAL before anything is launched (the table: include/llmi.h, llmi_kv_copy_rows)
int kv_copy_rows_check(const KvCopyArgs& a) {
    LLMI_REQUIRE(a.n_dst >= 1 && a.n_dst <= kKvCopyMaxDst, "kv_copy_rows: n_dst must be 1..7");
    LLMI_REQUIRE(a.layers > 0 && a.kv_heads > 0 && a.max_seq > 0,
                 "kv_copy_rows: layers, kv_heads and max_seq must be positive");
    LLMI_REQUIRE(a.n_rows >= 0 && a.n_rows <= a.max_seq, "kv_copy_rows: n_rows must be in [0, max_seq]");
    LLMI_REQUIRE(a.head_dim == 128, "kv_copy_rows: head_dim must be 128");
    LLMI_REQUIRE(a.cache_dtype == LLMI_F32 || a.cache_dtype == LLMI_F16 || a.cache_dtype == LLMI_I8,
                 "kv_copy_rows: cache dtype must be f32, f16 or i8");
    const bool q8 = a.cache_dtype == LLMI_I8;
    LLMI_REQUIRE(a.src_k && a.src_v, "kv_copy_rows: null source");
    LLMI_REQUIRE(!q8 || (a.src_k_scale && a.src_v_scale), "kv_copy_rows: an int8 cache needs its scales");
    // every buffer written is distinct from every other one and from the buffers read
    const void* seen[2 * (kKvCopyMaxDst + 1)] = {a.src_k, a.src_v};
    const void* seen_s[2 * (kKvCopyMaxDst + 1)] = {a.src_k_scale, a.src_v_scale};
    int ns = 2;
    LLMI_REQUIRE(aligned16(a.src_k) && aligned16(a.src_v) &&
                     (!q8 || (aligned16(a.src_k_scale) && aligned16(a.src_v_scale))),
                 "kv_copy_rows: buffers must be 16-byte aligned");
    for (int d = 0; d < a.n_dst; ++d) {
        LLMI_REQUIRE(a.dst_k[d] && a.dst_v[d], "kv_copy_rows: null destination");
        LLMI_REQUIRE(!q8 || (a.dst_k_scale[d] && a.dst_v_scale[d]), "kv_copy_rows: an int8 cache needs its scales");
        LLMI_REQUIRE(aligned16(a.dst_k[d]) && aligned16(a.dst_v[d]) &&
                         (!q8 || (aligned16(a.dst_k_scale[d]) && aligned16(a.dst_v_scale[d]))),
                     "kv_copy_rows: buffers must be 16-byte aligned");
        for (int w = 0; w < 2; ++w) {
            const void* p = w ? a.dst_v[d] : a.dst_k[d];
            const void* ps = w ? a.dst_v_scale[d] : a.dst_k_scale[d];
            for (int i = 0; i < ns; ++i) {
                LLMI_REQUIRE(p != seen[i], i < 2 ? "kv_copy_rows: a destination is the source"
                                                 : "kv_copy_rows: a destination appears twice");
                LLMI_REQUIRE(!q8 || ps != seen_s[i], i < 2 ? "kv_copy_rows: a destination is the source"
                                                           : "kv_copy_rows: a destination appears twice");
            }
            seen[ns] = p;
            seen_s[ns] = ps;
            ++ns;
        }
    }
    return LLMI_OK;
}

}  // namespace

int kv_copy_rows_launch(const KvCopyArgs& a, hipStream_t s) {
    LLMI_TRY(kv_copy_rows_check(a));
    if (a.n_rows == 0) return LLMI_OK;
    const bool q8 = a.cache_dtype == LLMI_I8;
    const size_t row_bytes = (size_t)a.head_dim * dtype_size(a.cache_dtype);
    KvCopyKernelArgs k{};
    k.src[0] = static_cast<const char*>(a.src_k);
    k.src[1] = static_cast<const char*>(a.src_v);
    k.src_s[0] = q8 ? static_cast<const unsigned short*>(a.src_k_scale) : nullptr;
    k.src_s[1] = q8 ? static_cast<const unsigned short*>(a.src_v_scale) : nullptr;
    for (int d = 0; d < a.n_dst; ++d) {
        k.dst[0][d] = static_cast<char*>(a.dst_k[d]);
        k.dst[1][d] = static_cast<char*>(a.dst_v[d]);
        k.dst_s[0][d] = q8 ? static_cast<unsigned short*>(a.dst_k_scale[d]) : nullptr;
        k.dst_s[1][d] = q8 ? static_cast<unsigned short*>(a.dst_v_scale[d]) : nullptr;
    }
    k.n_dst = a.n_dst;
    k.segs = a.layers * a.kv_heads;
    k.seg_stride = (size_t)a.max_seq * row_bytes;
    k.seg_bytes = (size_t)a.n_rows * row_bytes;
    k.chunks = (int)((k.seg_bytes + kCopyChunk - 1) / kCopyChunk);
    k.sc_stride = (size_t)a.max_seq;
    k.sc_n = (size_t)a.n_rows;
    int n_cu = a.n_cu;
    if (n_cu <= 0) {
        int dev = 0;
        LLMI_HIP(hipGetDevice(&dev));
        LLMI_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
    }
    const size_t items = (size_t)2 * k.segs * k.chunks + (q8 ? (size_t)2 * k.segs : 0);
    const int grid = (int)std::min<size_t>(items, (size_t)std::max(n_cu, 1) * kCopyWgPerCu);
    hipLaunchKernelGGL(kv_copy_rows_kernel, dim3(grid), dim3(kCopyT), 0, s, k);
    LLMI_HIP(hipGetLastError());
    return LLMI_OK;
}

}  // namespace llmi
