// The gfx950 device primitives of the hand-scheduled MFMA kernels: vector typedefs, the bf16 pack, buffer descriptors and
// compiler-tracked buffer access, inline-asm loads with their counted waits, and the LDS asm.  ONE copy, with what each of them
// has cost so far written next to it.  A primitive belongs here when two or more kernels use it with the same body; what one
// kernel alone uses stays beside that kernel.  Consumers say `using namespace sc2prim;` inside their own namespace.
#pragma once
#include "sc2_common.h"

#ifndef SC2_VMCAP
#define SC2_VMCAP 63   // DEBUG: -DSC2_VMCAP=<n> caps every counted wait_vm at n (0 = drain): bisects a wrong budget
#endif

namespace sc2prim {

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef const __attribute__((address_space(1))) void *gbl_ptr_t;
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ bf16 helpers
// one v_cvt_pk_bf16_f32 on an explicit (e0, e1) pair.  With scalar element-wise code the SLP vectoriser paired the wrong
// elements ((e0, e2), (e1, e3)) and re-interleaved them with and / shift / or_sdwa / v_mov: 870 vector instructions per wave for
// the in-place epilogue of a tile where 350 do (round 4).
__device__ __forceinline__ uint32_t pack2(f32x2_t v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t)); }
__device__ __forceinline__ uint32_t pack2(float a, float b) {   // one v_cvt_pk_bf16_f32
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}
__device__ __forceinline__ float bf_lo(uint32_t v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float bf_hi(uint32_t v) { return __builtin_bit_cast(float, v & 0xFFFF0000u); }

// ------------------------------------------------------------------------------------------------ compiler-tracked buffer access
// Buffer descriptors and buffer-addressed direct-to-LDS loads.  The host pass of hipcc parses kernel bodies too and has
// neither the type nor the builtins: it gets stand-ins (a kernel whose body fails to parse silently loses its host stub).
#if defined(__HIP_DEVICE_COMPILE__)
typedef __amdgpu_buffer_rsrc_t buf_rsrc_t;
__device__ __forceinline__ buf_rsrc_t make_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
// 16 bytes per lane from base + voff + soff (voff per lane, out of range -> zeros; soff scalar) to LDS at dst + 16 * lane
__device__ __forceinline__ void buf_load_lds16(buf_rsrc_t r, lds_ptr_t dst, uint32_t voff, uint32_t soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, (int)voff, (int)soff, 0, 0);
}
__device__ __forceinline__ uint4 buf_load16(buf_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
// A 16-byte buffer store reads its data registers for a few cycles after issue (lanes 12-15 of every 16 last): the GCN / CDNA
// hazard "VMEM store of more than 64 bits followed by a VALU write of its data VGPRs".  hipcc's hazard recogniser inserts the
// wait states only when the store's soffset field is NOT a register (GCNHazardRecognizer exempts MUBUF stores with an SGPR
// soffset) -- and every store here carries an SGPR soffset.  On gfx950 the hazard exists in that form too:
// tools/micro/store_hazard.hip issues `buffer_store_dwordx4 v[10:13], voff, rsrc, sN offen` directly followed by writes of
// v10..v13 and finds the NEW value in memory for 0.12 % of the elements, all of them in lanes 12-15 of a group of 16 (with a
// literal soffset, the case the compiler does handle: 6 %); ONE wait state removes every error (profiles/r04_store_hazard.txt).
// That is what round 2 saw in conv2x2_win.hip: hipcc scheduled a VALU write of a data register directly behind a store, and lanes
// 12-15 of the second wave of a SIMD (the one that is delayed at the memory pipe) stored the new value.  Two wait states follow
// every store here (what the compiler inserts for the literal-soffset form on gfx940+); the bit-exact multi-launch test
// (tests/test_gpu_kernels.py::test_conv2x2_win) stays in the default GPU suite as the guard against a compiler update, and
// tools/audit_vmcnt.py --stores checks the built ISA.  NT: non-temporal, the kernel's SC2_NT_<KERNEL> switch (sc2_common.h).
template <bool NT = false>
__device__ __forceinline__ void buf_store16(buf_rsrc_t r, uint32_t voff, uint32_t soff, u32x4_t v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)voff, (int)soff, NT ? SC2_BUF_AUX_NT : 0);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 1" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// 16-byte store through a descriptor, masked lanes sent out of range instead of branching around the store.  soffset is the
// LITERAL 0: that is the form for which hipcc inserts the wait states of the ">64-bit store data" hazard itself (with an SGPR
// soffset it does not: buf_store16 above, tools/micro/store_hazard.hip)
template <bool NT = false>
__device__ __forceinline__ void buf_store16_z(buf_rsrc_t r, uint32_t voff, uint4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{v.x, v.y, v.z, v.w}, r, (int)voff, 0, NT ? SC2_BUF_AUX_NT : 0);
}
#else   // host pass: stand-ins
typedef int buf_rsrc_t;
__device__ __forceinline__ buf_rsrc_t make_rsrc(const void *, uint32_t) { return 0; }
__device__ __forceinline__ void buf_load_lds16(buf_rsrc_t, lds_ptr_t, uint32_t, uint32_t) {}
__device__ __forceinline__ uint4 buf_load16(buf_rsrc_t, uint32_t, uint32_t) { return make_uint4(0, 0, 0, 0); }
template <bool NT = false>
__device__ __forceinline__ void buf_store16(buf_rsrc_t, uint32_t, uint32_t, u32x4_t) {}
template <bool NT = false>
__device__ __forceinline__ void buf_store16_z(buf_rsrc_t, uint32_t, uint4) {}
#endif

// ------------------------------------------------------------------------------------------------ inline-asm loads, counted waits
// Weight fragments are loaded by INLINE ASM and waited for with hand-counted `s_waitcnt vmcnt(N)` (round 4).  With the
// compiler's own loads the conditional window fills in front of a slab made its scoreboard merge conservative: the first
// k-step of every other slab of conv2x2_win.hip waited `vmcnt(2)`, i.e. for the window pieces of the NEXT slab issued a few
// instructions earlier (a full L2 / HBM round trip with every wave of the workgroup parked; tools/audit_vmcnt.py shows such waits).
// The asm loads are invisible to that scoreboard; vmcnt retires in issue order, so "all but the N youngest" is exact.
// Rules that keep this safe: (i) a fragment register is written by its load and read only by the MFMAs of its k-step,
// which sit behind wait_vm: every MFMA of a step consumes a pixel fragment that went through wait_lgkm (asm volatile, issued
// behind wait_vm in program order), so none can be placed above it; (ii) wait_vm does NOT name the registers: as a tied
// "+v" operand the compiler once placed a v_mov of the fragment into a fresh register IN FRONT of the wait -- a copy of a
// register whose load is still in flight (stale weights, found by the bit-exact multi-tile test); (iii) the load of k-step
// k + 4 goes into the registers of k-step k AFTER that step's last MFMA (no renaming); (iv) tools/audit_vmcnt.py --copies
// checks in the built ISA that no instruction but an MFMA reads a register written by such a load (tests/test_abi.py).
__device__ __forceinline__ i32x4_t rsrc_words(const void *base, uint32_t bytes) {   // raw buffer descriptor: base, no stride, size, 32-bit raw data format
    const uint64_t a = (uint64_t)(uintptr_t)base;
    return i32x4_t{(int)(uint32_t)a, (int)(uint32_t)((a >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}
// ("s_nop 4": the hazard recognizer does not look into inline asm.  The scalar offset / descriptor may have been written by a
//  VALU instruction just before -- hipcc restores spilled SGPRs with v_readlane_b32 -- and a VMEM instruction needs 5 wait states
//  behind a VALU write of an SGPR it reads: without them the loads of the tail-mode kernel used a stale offset (wrong weights) and
//  conv1x1_win a stale descriptor (memory fault).)
__device__ __forceinline__ void wload16(u32x4_t &d, i32x4_t r, uint32_t voff, uint32_t soff) {   // ("; wfrag": marker for the audit)
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen ; wfrag" : "=&v"(d) : "v"(voff), "s"(r), "s"(soff) : "memory");
}
__device__ __forceinline__ void cload16(u32x4_t &d, i32x4_t r, uint32_t voff, uint32_t soff) {   // epilogue constants (wait_vm_tied)
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen" : "=&v"(d) : "v"(voff), "s"(r), "s"(soff) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {   // (does not name the fragment registers: rule (ii))
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < SC2_VMCAP ? N : SC2_VMCAP) : "memory");
}
// (epilogue constants only: consumed by vector ALU code, which nothing else orders behind the wait.  Their loads are at least
//  eight k-steps old at the wait, so even a copy placed in front of it reads landed data)
template <int N>
__device__ __forceinline__ void wait_vm_tied(u32x4_t &a, u32x4_t &b) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
// wait until at most N of this wave's LDS operations are outstanding; `v` (the destination of the read being waited for)
// is threaded through so that its consumers cannot be scheduled above the wait
template <int N>
__device__ __forceinline__ void wait_lgkm(u32x4_t &v) {
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}

// ------------------------------------------------------------------------------------------------ LDS asm
// LDS accesses the compiler must not see: hipcc knows that a direct-to-LDS load writes LDS and drains vmcnt(0) in front of every
// LDS access it can see behind one (may-alias).  lgkmcnt retires in order: results are consumed behind wait_lgkm.
__device__ __forceinline__ uint4 lds_read16(uint32_t addr) {
    uint4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// (V: conv_dec_persist.hip reads into uint4 -- as an asm output the struct and the vector are NOT the same to hipcc: its K loop gets
//  another schedule with u32x4_t)
template <int OFF, class V = u32x4_t>
__device__ __forceinline__ V lds_read16_imm(uint32_t addr) {
    V v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void lds_write16(uint32_t addr, u32x4_t v) {
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write16(uint32_t addr, uint4 v) {
    const u32x4_t q = {v.x, v.y, v.z, v.w};
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(q) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write16_imm(uint32_t addr, u32x4_t v) {
    asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}

}  // namespace sc2prim
