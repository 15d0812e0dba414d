// Cache policy of bulk global accesses, chosen per site by a compile-time tag.  Each XCD's L2 is write-back and not coherent with the other seven, so
// a kernel that ends with dirty lines ends with their write-back; a write-through store (sc1) sends its bytes on while the kernel still computes and
// drops the line from the writer's L2, a non-temporal access (nt) keeps the line but marks it first to go.  Every form is one the compiler sees and
// counts in vmcnt.  Values and addresses do not depend on the tag: a site is switched by changing one template argument.
// In use (profiles/r20_store_policy.md has what each candidate site measured): write-through 4-byte stores for the split-K and weight-gradient slabs (EpiSlab,
// actor_fc1.hip, conv1_wgrad.hip, conv23_wgrad.hip), non-temporal 16-byte stores for the actor step's replay rows (encoder_fused.hip).  The 16-byte write-through
// form and the non-temporal loads were tried on the encoder's activations, the data gradients, the optimizer tail and the learner's frame fetches and gained
// nothing there; they stay here for the next site that wants trying.
#pragma once
#include "a0_defs.h"

struct a0_st_plain {};      // the default policy
struct a0_st_wt {};         // write-through: buffer_store_dwordx4 ... sc1 for 16 bytes, global_store ... sc0 sc1 for 4 and 8
struct a0_st_nt {};         // non-temporal: global_store / global_load ... nt

#if defined(__HIPCC__)

typedef uint32_t a0_u4v __attribute__((ext_vector_type(4)));
typedef uint32_t a0_u2v __attribute__((ext_vector_type(2)));

template <class POL> inline constexpr bool a0_is_wt = false;
template <> inline constexpr bool a0_is_wt<a0_st_wt> = true;
template <class POL> inline constexpr bool a0_is_nt = false;
template <> inline constexpr bool a0_is_nt<a0_st_nt> = true;

A0_D a0_u4v a0_bits16(const a0_f4& v) { return a0_u4v{__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)}; }
A0_D a0_u4v a0_bits16(const uint4& v) { return a0_u4v{v.x, v.y, v.z, v.w}; }

// A block of `bytes` bytes at a WAVE-UNIFORM base (an observation's activation block, an env's replay row, a slab, a flat parameter buffer — never the
// replay ring: offsets are 32 bits) that lanes fill 16 bytes at a time.  The write-through form is a buffer resource in four scalar registers whose
// range check drops a store at or beyond `bytes`; the base may have any 4-byte alignment.  readfirstlane makes the uniformity visible to the compiler.
template <class POL>
struct a0_out16 {
    float* base;
    A0_D a0_out16(float* b, unsigned) : base(b) {}
    template <class V> A0_D void put(unsigned i, const V& v) const {       // 16 bytes at float i of the block (i a multiple of four)
        if constexpr (a0_is_nt<POL>) __builtin_nontemporal_store(a0_bits16(v), (a0_u4v*)(base + i));
        else *(V*)(base + i) = v;
    }
};
template <>
struct a0_out16<a0_st_wt> {
    __amdgpu_buffer_rsrc_t rsrc;
    A0_D a0_out16(float* b, unsigned bytes) {
        const uintptr_t a = (uintptr_t)b;
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
        rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(((uintptr_t)hi << 32) | lo), 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
    }
    template <class V> A0_D void put(unsigned i, const V& v) const { __builtin_amdgcn_raw_buffer_store_b128(a0_bits16(v), rsrc, (int)(i << 2), 0, 16); }
};

// 8 and 4 bytes per lane at any address
template <class POL> A0_D void a0_store8(void* p, const uint2& v) {
    if constexpr (a0_is_wt<POL>) __hip_atomic_store((unsigned long long*)p, (unsigned long long)v.x | ((unsigned long long)v.y << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if constexpr (a0_is_nt<POL>) __builtin_nontemporal_store(a0_u2v{v.x, v.y}, (a0_u2v*)p);
    else *(uint2*)p = v;
}
template <class POL> A0_D void a0_store4(void* p, uint32_t v) {
    if constexpr (a0_is_wt<POL>) __hip_atomic_store((uint32_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else if constexpr (a0_is_nt<POL>) __builtin_nontemporal_store(v, (uint32_t*)p);
    else *(uint32_t*)p = v;
}
// 16 bytes per lane at any address, for outputs without a uniform base within 4 GB: there is no write-through form of it
template <class POL, class V> A0_D void a0_store16(V* p, const V& v) {
    static_assert(!a0_is_wt<POL>, "write-through 16-byte stores go through a0_out16");
    if constexpr (a0_is_nt<POL>) __builtin_nontemporal_store(a0_bits16(v), (a0_u4v*)p);
    else *p = v;
}

// a once-read load of 16 or 4 bytes (plain and non-temporal; write-through does not apply to loads)
template <class POL> A0_D uint4 a0_load16(const void* p) {
    static_assert(!a0_is_wt<POL>, "loads are plain or non-temporal");
    if constexpr (a0_is_nt<POL>) { const a0_u4v v = __builtin_nontemporal_load((const a0_u4v*)p); return uint4{v.x, v.y, v.z, v.w}; }
    else return *(const uint4*)p;
}
template <class POL> A0_D uint32_t a0_load4(const void* p) {
    static_assert(!a0_is_wt<POL>, "loads are plain or non-temporal");
    if constexpr (a0_is_nt<POL>) return __builtin_nontemporal_load((const uint32_t*)p);
    else return *(const uint32_t*)p;
}
#endif

// one float of an epilogue that the host emulation evaluates too (operands.h, net_impl.h): there it is a plain store
template <class POL> A0_HD void a0_put_f32(float* p, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    a0_store4<POL>(p, __float_as_uint(v));
#else
    *p = v;
#endif
}
