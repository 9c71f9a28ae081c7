// zj_ubench.hip -- instruction-issue micro-benchmarks for gfx950 integer VALU ops (tools/ubench.py).
// Every variant executes, per loop iteration, 8 asm statements of 8 independent instructions each
// (64 instructions on 8 registers), written in inline asm so the compiler can neither fold nor
// re-select them.  Not part of the decode path.
#include <hip/hip_runtime.h>

#include "zj_lab_launch.h"

namespace zj {

#define R8(x) x x x x x x x x

#define UB_KERNEL(NAME, INSTR)                                                                         \
    __global__ __launch_bounds__(256) void NAME(int* out, int iters, int seed)                         \
    {                                                                                                  \
        int a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, \
            a6 = a0 * 17, a7 = a0 * 19;                                                                \
        int k = __builtin_amdgcn_readfirstlane(seed | 3);                                              \
        int b = a0 ^ 0x55aa;                                                                           \
        for (int it = 0; it < iters; it++) {                                                           \
            R8(asm volatile(INSTR(%0) INSTR(%1) INSTR(%2) INSTR(%3) INSTR(%4) INSTR(%5) INSTR(%6) INSTR(%7) \
                            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) \
                            : "s"(k), "v"(b));)                                                        \
        }                                                                                              \
        int acc = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                               \
        if (acc == 0x7fffffff) out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                       \
    }

// %8 = SGPR k, %9 = VGPR b
#define I_ADD(r) "v_add_u32_e32 " #r ", %9, " #r "\n"
#define I_ADD64(r) "v_add_u32_e64 " #r ", %9, " #r "\n"
#define I_ADDS(r) "v_add_u32_e32 " #r ", %8, " #r "\n"
#define I_MULLO(r) "v_mul_lo_u32 " #r ", " #r ", %8\n"
#define I_MUL24(r) "v_mul_i32_i24_e32 " #r ", %8, " #r "\n"
#define I_MUL24L(r) "v_mul_i32_i24_e32 " #r ", 0x14e8, " #r "\n"
#define I_MAD24S(r) "v_mad_i32_i24 " #r ", " #r ", %8, %9\n"
#define I_MAD24V(r) "v_mad_i32_i24 " #r ", " #r ", %9, %9\n"
#define I_MAD24VV(r) "v_mad_i32_i24 " #r ", " #r ", %9, " #r "\n"
#define I_ASHR(r) "v_ashrrev_i32_e32 " #r ", 3, " #r "\n"
#define I_LSHLADD(r) "v_lshl_add_u32 " #r ", " #r ", 3, %9\n"
#define I_ADD3(r) "v_add3_u32 " #r ", " #r ", %9, %8\n"
#define I_MED3(r) "v_med3_i32 " #r ", " #r ", 0, %8\n"
#define I_PERM(r) "v_perm_b32 " #r ", " #r ", %9, %8\n"
#define I_PKADD(r) "v_pk_add_u16 " #r ", " #r ", %9\n"
#define I_PKMUL(r) "v_pk_mul_lo_u16 " #r ", " #r ", %9\n"
#define I_PKMAD(r) "v_pk_mad_u16 " #r ", " #r ", %9, %9\n"
#define I_PKASHR(r) "v_pk_ashrrev_i16 " #r ", 2, " #r "\n"
#define I_PKMAX(r) "v_pk_max_i16 " #r ", " #r ", %9\n"
#define I_SDWA(r) "v_mul_i32_i24_sdwa " #r ", %8, sext(" #r ") dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n"
#define I_LSHLOR(r) "v_lshl_or_b32 " #r ", " #r ", 8, %9\n"
#define I_ANDOR(r) "v_and_or_b32 " #r ", " #r ", %8, %9\n"
#define I_ALIGN(r) "v_alignbit_b32 " #r ", " #r ", %9, 16\n"
#define I_BFE(r) "v_bfe_i32 " #r ", " #r ", 0, 16\n"
#define I_MOV(r) "v_mov_b32_e32 " #r ", %9\n"
#define I_CNDMASK(r) "v_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_OR(r) "v_or_b32_e32 " #r ", %9, " #r "\n"
#define I_SUB(r) "v_sub_u32_e32 " #r ", " #r ", %9\n"
#define I_MADU16(r) "v_mad_i32_i16 " #r ", " #r ", %9, %9\n"
#define I_SATPK(r) "v_sat_pk_u8_i16_e32 " #r ", " #r "\n"
#define I_MAD_U32_U24(r) "v_mad_u32_u24 " #r ", " #r ", %8, %9\n"
#define I_PKSUB(r) "v_pk_sub_i16 " #r ", " #r ", %9\n"
#define I_PKMIN(r) "v_pk_min_i16 " #r ", " #r ", %9\n"
#define I_OR3(r) "v_or3_b32 " #r ", " #r ", %9, %8\n"
#define I_MIX1(r) "v_mul_i32_i24_e32 " #r ", 0x14e8, " #r "\n v_add_u32_e32 " #r ", %9, " #r "\n"
#define I_MIX2(r) "v_mad_i32_i24 " #r ", " #r ", %9, %9\n v_add_u32_e32 " #r ", %9, " #r "\n v_ashrrev_i32_e32 " #r ", 3, " #r "\n"
#define I_MIX3(r) "v_add_u32_e32 " #r ", %9, " #r "\n v_ashrrev_i32_e32 " #r ", 3, " #r "\n"
#define I_MAX(r) "v_max_i32_e32 " #r ", %9, " #r "\n"
#define I_LSHL(r) "v_lshlrev_b32_e32 " #r ", 3, " #r "\n"
#define I_AND(r) "v_and_b32_e32 " #r ", %9, " #r "\n"
// round 2: the packed IDCT's instructions
#define I_DOT2C(r) "v_dot2c_i32_i16_e32 " #r ", 0x08a914e8, %9\n"
#define I_DOT2CS(r) "v_dot2c_i32_i16_e32 " #r ", %8, %9\n"
#define I_DOT2(r) "v_dot2_i32_i16 " #r ", %9, %8, " #r "\n"
#define I_DOT2Z(r) "v_dot2_i32_i16 " #r ", " #r ", %8, 0\n"
#define I_SAD16(r) "v_sad_u16 " #r ", %9, %8, " #r "\n"
#define I_ASHR_SDWA(r) "v_ashrrev_i32_sdwa " #r ", %8, %9 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n"
#define I_ASHRS(r) "v_ashrrev_i32_e32 " #r ", %8, " #r "\n"
#define I_SATPK_SDWA(r) "v_sat_pk_u8_i16_sdwa " #r ", %9 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD\n"
#define I_MIX_DOT(r) "v_dot2c_i32_i16_e32 " #r ", 0x08a914e8, %9\n v_add_u32_e32 " #r ", %9, " #r "\n"

// the byte formulation of the chroma up-sampling filters: four byte averages per instruction, and the byte funnel shift
#define I_LERP(r) "v_lerp_u8 " #r ", " #r ", %9, %8\n"
#define I_LERPZ(r) "v_lerp_u8 " #r ", " #r ", %9, 0\n"
#define I_ALIGNBYTE(r) "v_alignbyte_b32 " #r ", " #r ", %9, 1\n"

UB_KERNEL(ub_add, I_ADD)
UB_KERNEL(ub_add64, I_ADD64)
UB_KERNEL(ub_adds, I_ADDS)
UB_KERNEL(ub_mullo, I_MULLO)
UB_KERNEL(ub_mul24, I_MUL24)
UB_KERNEL(ub_mul24l, I_MUL24L)
UB_KERNEL(ub_mad24s, I_MAD24S)
UB_KERNEL(ub_mad24v, I_MAD24V)
UB_KERNEL(ub_mad24vv, I_MAD24VV)
UB_KERNEL(ub_ashr, I_ASHR)
UB_KERNEL(ub_lshladd, I_LSHLADD)
UB_KERNEL(ub_add3, I_ADD3)
UB_KERNEL(ub_med3, I_MED3)
UB_KERNEL(ub_perm, I_PERM)
UB_KERNEL(ub_pkadd, I_PKADD)
UB_KERNEL(ub_pkmul, I_PKMUL)
UB_KERNEL(ub_pkmad, I_PKMAD)
UB_KERNEL(ub_pkashr, I_PKASHR)
UB_KERNEL(ub_pkmax, I_PKMAX)
UB_KERNEL(ub_sdwa, I_SDWA)
UB_KERNEL(ub_lshlor, I_LSHLOR)
UB_KERNEL(ub_andor, I_ANDOR)
UB_KERNEL(ub_align, I_ALIGN)
UB_KERNEL(ub_bfe, I_BFE)
UB_KERNEL(ub_mov, I_MOV)
UB_KERNEL(ub_cndmask, I_CNDMASK)
UB_KERNEL(ub_or, I_OR)
UB_KERNEL(ub_sub, I_SUB)
UB_KERNEL(ub_madi16, I_MADU16)
UB_KERNEL(ub_satpk, I_SATPK)
UB_KERNEL(ub_madu24, I_MAD_U32_U24)
UB_KERNEL(ub_pksub, I_PKSUB)
UB_KERNEL(ub_pkmin, I_PKMIN)
UB_KERNEL(ub_or3, I_OR3)
UB_KERNEL(ub_mix1, I_MIX1)
UB_KERNEL(ub_mix2, I_MIX2)
UB_KERNEL(ub_mix3, I_MIX3)
UB_KERNEL(ub_max, I_MAX)
UB_KERNEL(ub_lshl, I_LSHL)
UB_KERNEL(ub_and, I_AND)
UB_KERNEL(ub_dot2c, I_DOT2C)
UB_KERNEL(ub_dot2cs, I_DOT2CS)
UB_KERNEL(ub_dot2, I_DOT2)
UB_KERNEL(ub_dot2z, I_DOT2Z)
UB_KERNEL(ub_sad16, I_SAD16)
UB_KERNEL(ub_ashr_sdwa, I_ASHR_SDWA)
UB_KERNEL(ub_ashrs, I_ASHRS)
UB_KERNEL(ub_satpk_sdwa, I_SATPK_SDWA)
UB_KERNEL(ub_mix_dot, I_MIX_DOT)
UB_KERNEL(ub_lerp, I_LERP)
UB_KERNEL(ub_lerpz, I_LERPZ)
UB_KERNEL(ub_alignbyte, I_ALIGNBYTE)

#define UB_KERNEL_BODY(NAME, BODY)                                                                     \
    __global__ __launch_bounds__(256) void NAME(int* out, int iters, int seed)                         \
    {                                                                                                  \
        int a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, \
            a6 = a0 * 17, a7 = a0 * 19;                                                                \
        int k = __builtin_amdgcn_readfirstlane(seed | 3);                                              \
        int b = a0 ^ 0x55aa;                                                                           \
        for (int it = 0; it < iters; it++) {                                                           \
            R8(asm volatile(BODY                                                                       \
                            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) \
                            : "s"(k), "v"(b));)                                                        \
        }                                                                                              \
        int acc = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                               \
        if (acc == 0x7fffffff) out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                       \
    }
#define ALL8(I) I(%0) I(%1) I(%2) I(%3) I(%4) I(%5) I(%6) I(%7)
// 24 instructions per statement: 8 mad + 8 add + 8 ashr, grouped by kind vs interleaved per register
UB_KERNEL_BODY(ub_grp_mad_add_ashr, ALL8(I_MAD24V) ALL8(I_ADD) ALL8(I_ASHR))
UB_KERNEL_BODY(ub_grp_mad_add2, ALL8(I_MAD24V) ALL8(I_ADD) ALL8(I_SUB) ALL8(I_ASHR) ALL8(I_OR))
UB_KERNEL_BODY(ub_grp_mad4_add4, I_MAD24V(%0) I_MAD24V(%1) I_MAD24V(%2) I_MAD24V(%3) I_ADD(%4) I_ADD(%5) I_ADD(%6) I_ADD(%7) I_MAD24V(%4) I_MAD24V(%5) I_MAD24V(%6) I_MAD24V(%7) I_ADD(%0) I_ADD(%1) I_ADD(%2) I_ADD(%3))
UB_KERNEL_BODY(ub_grp_mad2_add2, I_MAD24V(%0) I_MAD24V(%1) I_ADD(%2) I_ADD(%3) I_MAD24V(%4) I_MAD24V(%5) I_ADD(%6) I_ADD(%7) I_MAD24V(%2) I_MAD24V(%3) I_ADD(%0) I_ADD(%1) I_MAD24V(%6) I_MAD24V(%7) I_ADD(%4) I_ADD(%5))
UB_KERNEL_BODY(ub_grp_mad1_add1_indep, I_MAD24V(%0) I_ADD(%1) I_MAD24V(%2) I_ADD(%3) I_MAD24V(%4) I_ADD(%5) I_MAD24V(%6) I_ADD(%7) I_MAD24V(%1) I_ADD(%0) I_MAD24V(%3) I_ADD(%2) I_MAD24V(%5) I_ADD(%4) I_MAD24V(%7) I_ADD(%6))
UB_KERNEL_BODY(ub_grp_mad1_add3, I_MAD24V(%0) I_ADD(%1) I_ADD(%2) I_ADD(%3) I_MAD24V(%4) I_ADD(%5) I_ADD(%6) I_ADD(%7) I_MAD24V(%1) I_ADD(%0) I_ADD(%2) I_ADD(%3) I_MAD24V(%5) I_ADD(%4) I_ADD(%6) I_ADD(%7))

// round 5: what does a select cost?  (v_cndmask_b32_e32 on an untouched vcc measured 21 cycles in round 1 -- real, or the
// benchmark's?)  The same 64-instruction loop with a 64-bit lane mask in an SGPR pair as operand %10, vcc written once
// in front of the loop, and the idioms that could stand in for a select.
#define UB_KERNEL_M(NAME, INSTR)                                                                       \
    __global__ __launch_bounds__(256) void NAME(int* out, int iters, int seed)                         \
    {                                                                                                  \
        int a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, \
            a6 = a0 * 17, a7 = a0 * 19;                                                                \
        int k = __builtin_amdgcn_readfirstlane(seed | 3);                                              \
        int b = a0 ^ 0x55aa;                                                                           \
        const unsigned long long m = 0x5a5a33cc0ff0aa55ull ^ (unsigned long long)k;                    \
        asm volatile("s_mov_b64 vcc, %0" : : "s"(m) : "vcc");                                          \
        for (int it = 0; it < iters; it++) {                                                           \
            R8(asm volatile(INSTR(%0) INSTR(%1) INSTR(%2) INSTR(%3) INSTR(%4) INSTR(%5) INSTR(%6) INSTR(%7) \
                            : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) \
                            : "s"(k), "v"(b), "s"(m) : "vcc");)                                        \
        }                                                                                              \
        int acc = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;                                               \
        if (acc == 0x7fffffff) out[blockIdx.x * blockDim.x + threadIdx.x] = acc;                       \
    }
#define I_CND_VCC(r) "v_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_CND_S64(r) "v_cndmask_b32_e64 " #r ", " #r ", %9, %10\n"
#define I_CND_S64_K(r) "v_cndmask_b32_e64 " #r ", 0, 1, %10\n"
#define I_BFI(r) "v_bfi_b32 " #r ", %9, " #r ", %9\n"
#define I_CMP_CND(r) "v_cmp_gt_i32_e32 vcc, %9, " #r "\nv_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_CMP_S(r) "v_cmp_gt_i32_e64 s[20:21], %9, " #r "\n"
UB_KERNEL_M(ub_cnd_vcc, I_CND_VCC)
UB_KERNEL_M(ub_cnd_s64, I_CND_S64)
UB_KERNEL_M(ub_cnd_s64k, I_CND_S64_K)
UB_KERNEL_M(ub_bfi, I_BFI)
UB_KERNEL_M(ub_cmp_cnd, I_CMP_CND)
// which use of vcc is the slow one: a second select on the same compare?  a select with another instruction between it
// and its compare?  a select on a vcc that the scalar unit wrote?
#define I_CMP_CND2(r) "v_cmp_gt_i32_e32 vcc, %9, " #r "\nv_cndmask_b32_e32 " #r ", " #r ", %9, vcc\nv_cndmask_b32_e32 " #r ", %9, " #r ", vcc\n"
#define I_CMP_X_CND(r) "v_cmp_gt_i32_e32 vcc, %9, " #r "\nv_add_u32_e32 " #r ", %9, " #r "\nv_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_CMP_X3_CND(r) "v_cmp_gt_i32_e32 vcc, %9, " #r "\nv_add_u32_e32 " #r ", %9, " #r "\nv_sub_u32_e32 " #r ", " #r ", %9\nv_or_b32_e32 " #r ", %9, " #r "\nv_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_SVCC_CND(r) "s_mov_b64 vcc, %10\nv_cndmask_b32_e32 " #r ", " #r ", %9, vcc\n"
#define I_CMP64_CND2(r) "v_cmp_gt_i32_e64 s[20:21], %9, " #r "\nv_cndmask_b32_e64 " #r ", " #r ", %9, s[20:21]\nv_cndmask_b32_e64 " #r ", %9, " #r ", s[20:21]\n"
#define I_DPP_SHR(r) "v_mov_b32_dpp " #r ", %9 row_shr:1 row_mask:0xf bank_mask:0xf\n"
#define I_DPP_SHL_SELF(r) "v_mov_b32_dpp " #r ", " #r " row_shl:1 row_mask:0xf bank_mask:0xf\n"
#define I_DPP_ADD(r) "v_add_u32_dpp " #r ", %9, " #r " row_shr:1 row_mask:0xf bank_mask:0xf\n"
#define I_DS_SWZ(r) "ds_swizzle_b32 " #r ", " #r " offset:swizzle(SWAP,1)\ns_waitcnt lgkmcnt(0)\n"
UB_KERNEL_M(ub_dpp_shr, I_DPP_SHR)
UB_KERNEL_M(ub_dpp_shl_self, I_DPP_SHL_SELF)
UB_KERNEL_M(ub_dpp_add, I_DPP_ADD)
UB_KERNEL_M(ub_cmp_cnd2, I_CMP_CND2)
UB_KERNEL_M(ub_cmp_x_cnd, I_CMP_X_CND)
UB_KERNEL_M(ub_cmp_x3_cnd, I_CMP_X3_CND)
UB_KERNEL_M(ub_svcc_cnd, I_SVCC_CND)
__global__ __launch_bounds__(256) void ub_cmp64_cnd2(int* out, int iters, int seed)
{
    int a0 = seed + threadIdx.x, a1 = a0 * 3, a2 = a0 * 5, a3 = a0 * 7, a4 = a0 * 11, a5 = a0 * 13, a6 = a0 * 17, a7 = a0 * 19;
    int k = __builtin_amdgcn_readfirstlane(seed | 3);
    int b = a0 ^ 0x55aa;
    const unsigned long long m = 0x5a5a33cc0ff0aa55ull ^ (unsigned long long)k;
    for (int it = 0; it < iters; it++) {
        R8(asm volatile(I_CMP64_CND2(%0) I_CMP64_CND2(%1) I_CMP64_CND2(%2) I_CMP64_CND2(%3) I_CMP64_CND2(%4) I_CMP64_CND2(%5) I_CMP64_CND2(%6) I_CMP64_CND2(%7)
                        : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                        : "s"(k), "v"(b), "s"(m) : "s20", "s21");)
    }
    int acc = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7;
    if (acc == 0x7fffffff) out[blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

// shader-clock probe: cycles (s_memtime) spent by one wave in a fixed spin, to convert ms -> MHz
__global__ void ub_clock(unsigned long long* out, int iters)
{
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    int a = threadIdx.x;
    for (int i = 0; i < iters; i++) asm volatile(R8("v_add_u32_e32 %0, 1, %0\n") : "+v"(a));
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0 + (a == 0x7fffffff);
}

typedef void (*ub_fn)(int*, int, int);
static const struct { const char* name; ub_fn fn; } UB[] = {
    {"v_add_u32_e32 v,v,v", ub_add}, {"v_add_u32_e64 v,v,v", ub_add64}, {"v_add_u32_e32 v,s,v", ub_adds},
    {"v_sub_u32_e32", ub_sub}, {"v_or_b32_e32", ub_or}, {"v_mov_b32_e32", ub_mov}, {"v_ashrrev_i32_e32", ub_ashr},
    {"v_cndmask_b32_e32", ub_cndmask},
    {"v_mul_lo_u32 v,v,s", ub_mullo}, {"v_mul_i32_i24_e32 v,s,v", ub_mul24}, {"v_mul_i32_i24_e32 v,lit,v", ub_mul24l},
    {"v_mul_i32_i24_sdwa v,s,sext(v.w1)", ub_sdwa},
    {"v_mad_i32_i24 v,v,s,v", ub_mad24s}, {"v_mad_i32_i24 v,v,v,v(2 regs)", ub_mad24v}, {"v_mad_i32_i24 v,v,v,v(self)", ub_mad24vv},
    {"v_mad_u32_u24 v,v,s,v", ub_madu24}, {"v_mad_i32_i16 v,v,v,v", ub_madi16},
    {"v_lshl_add_u32", ub_lshladd}, {"v_add3_u32", ub_add3}, {"v_or3_b32", ub_or3}, {"v_med3_i32", ub_med3},
    {"v_perm_b32", ub_perm}, {"v_lshl_or_b32", ub_lshlor}, {"v_and_or_b32", ub_andor}, {"v_alignbit_b32", ub_align},
    {"v_bfe_i32", ub_bfe}, {"v_sat_pk_u8_i16", ub_satpk},
    {"v_pk_add_u16", ub_pkadd}, {"v_pk_sub_i16", ub_pksub}, {"v_pk_mul_lo_u16", ub_pkmul}, {"v_pk_mad_u16", ub_pkmad},
    {"v_pk_ashrrev_i16", ub_pkashr}, {"v_pk_max_i16", ub_pkmax}, {"v_pk_min_i16", ub_pkmin},
    {"v_max_i32_e32", ub_max}, {"v_lshlrev_b32_e32", ub_lshl}, {"v_and_b32_e32", ub_and},
    {"v_dot2c_i32_i16_e32 v,lit,v", ub_dot2c}, {"v_dot2c_i32_i16_e32 v,s,v", ub_dot2cs}, {"v_dot2_i32_i16 v,v,s,v", ub_dot2},
    {"v_dot2_i32_i16 v,v,s,0", ub_dot2z}, {"v_sad_u16 v,v,s,v", ub_sad16},
    {"v_ashrrev_i32_sdwa (word_1, preserve)", ub_ashr_sdwa}, {"v_ashrrev_i32_e32 v,s,v", ub_ashrs},
    {"v_sat_pk_u8_i16_sdwa (word_1, preserve)", ub_satpk_sdwa},
    {"v_lerp_u8 v,v,v,s", ub_lerp}, {"v_lerp_u8 v,v,v,0", ub_lerpz}, {"v_alignbyte_b32 v,v,v,1", ub_alignbyte},
    {"PAIR dot2c ; add          (2 instr)", ub_mix_dot},
    {"PAIR mul24 ; add          (2 instr)", ub_mix1}, {"TRIPLE mad24 ; add ; ashr (3 instr)", ub_mix2}, {"PAIR add ; ashr            (2 instr)", ub_mix3},
    {"GROUPED 8 mad | 8 add | 8 ashr   (x3 instr)", ub_grp_mad_add_ashr},
    {"GROUPED 8 mad | 32 simple        (x5 instr)", ub_grp_mad_add2},
    {"RUNS 4 mad | 4 add (indep)        (x2 instr)", ub_grp_mad4_add4},
    {"RUNS 2 mad | 2 add (indep)        (x2 instr)", ub_grp_mad2_add2},
    {"RUNS 1 mad | 1 add (indep)        (x2 instr)", ub_grp_mad1_add1_indep},
    {"RUNS 1 mad | 3 add (indep)        (x2 instr)", ub_grp_mad1_add3},
    {"v_cndmask_b32_e32 v,v,v,vcc (vcc set once)", ub_cnd_vcc}, {"v_cndmask_b32_e64 v,v,v,s[n:n+1]", ub_cnd_s64},
    {"v_cndmask_b32_e64 v,0,1,s[n:n+1]", ub_cnd_s64k}, {"v_bfi_b32 v,v,v,v", ub_bfi},
    {"PAIR v_cmp_gt_i32 vcc ; v_cndmask vcc (2 instr)", ub_cmp_cnd},
    {"v_cmp vcc ; cndmask vcc ; cndmask vcc (3 instr)", ub_cmp_cnd2}, {"v_cmp vcc ; v_add ; cndmask vcc (3 instr)", ub_cmp_x_cnd},
    {"v_cmp vcc ; add ; sub ; or ; cndmask vcc (5 instr)", ub_cmp_x3_cnd}, {"s_mov vcc ; cndmask vcc (1 VALU)", ub_svcc_cnd},
    {"v_cmp_e64 s[20:21] ; cndmask_e64 x2 s[20:21] (3 instr)", ub_cmp64_cnd2},
    {"v_mov_b32_dpp v,v row_shr:1", ub_dpp_shr}, {"v_mov_b32_dpp v,v(self) row_shl:1 (dependent)", ub_dpp_shl_self}, {"v_add_u32_dpp v,v,v row_shr:1", ub_dpp_add},
};

int ubench2_count() { return (int)(sizeof(UB) / sizeof(UB[0])); }
const char* ubench2_name(int op) { return (op >= 0 && op < ubench2_count()) ? UB[op].name : ""; }
hipError_t launch_ubench2(int op, int* out, int blocks, int iters, int seed, hipStream_t s)
{
    if (op < 0 || op >= ubench2_count()) return hipErrorInvalidValue;
    hipLaunchKernelGGL(UB[op].fn, dim3(blocks), dim3(256), 0, s, out, iters, seed);
    return hipGetLastError();
}
hipError_t launch_ub_clock(unsigned long long* out, int blocks, int iters, hipStream_t s)
{
    hipLaunchKernelGGL(ub_clock, dim3(blocks), dim3(64), 0, s, out, iters);
    return hipGetLastError();
}

} // namespace zj
