#!/usr/bin/env python3
"""Generate timewarp_amd/csrc/tw_h3_attnd_asm.inc: the hand-scheduled dense-softmax attention block of one encoder layer of
the split-fp16 net-block kernel (transformer_nvp: nn.MultiheadAttention with 8 heads of 16, 48 tokens per wave, gfx950).

Dataflow (everything in registers):
  q_h, k_h = W_{q,k}[16 h ..] . x^T   standard orientation, D tile [feature][token] = K = 16 MFMA operand layout
  v_h      = x . W_v[16 h ..]^T       operands swapped: D tile [token][feature], lane = feature = A operand of P.V
  S^T[key][query] = k_h q_h^T / 4 (K = 16 MFMAs, 3-term split), masked softmax in the accumulator registers,
  O^T = V^T P^T (K = 32 for key tiles 0, 1 + K = 16 for tile 2), two heads' O = one k-step of out_proj.

Schedule - one wave per SIMD, so VALU work only hides in the shadow of MFMAs; per head h:
  A  stage V(h)               36 MFMAs  |  scale / bias / split of q_h, k_h               72 VALU
  B  S(h)                     27 MFMAs  |  scale / bias / split of v_h                    36 VALU
  C  stages Q(h+1), K(h+1)    72 MFMAs  |  mask, max, exp, sum, split of P(h)            ~330 VALU   (bare after the last head)
  D  P.V(h)                   18 MFMAs  |  1/sum, split of O(h)                           48 VALU
  E  (odd h) out_proj stages  72 MFMAs
The accumulators of q / k / v are single-buffered: their consumers (the splits) are done before the next head's stage
writes them.  Weight-stage order in the stream (h3_pack_weights, dense branch):  q0 k0 | v_h  q_{h+1} k_{h+1}  [out_proj of
the pair after an odd h] ...  Stage hand-off, ring and DMA protocol as in gen_h3_attn_asm.py.

Register map (private to the asm statement):
  v0..v31    weight tile slots p = 0..3: hi v[8p..], lo v[8p+4..]
  v32..v67   accumulators QA[jt] KA[jt] VA[jt]
  v68..v91   q / k operands (K = 16): QH QL KH KL [jt] x 2 registers
  v92..v103  v operands: VH01 VL01 (K = 32, key tiles 0 and 1), VH2 VL2 (K = 16, tile 2)
  v104..v139 S^T accumulators SC[jt][mt]; P operands are written over them: PL01 (+0), PH01 (+4), PL2 (+8), PH2 (+10)
  v140..v142 1 / sum per query tile; v144..v167 O32[jt], O16[jt]; v168..v191 out_proj operand OB[jt] = {h 4, l 4}
  v192..v203 temporaries; v204..v211 bias registers; v212.. addresses
  a0..a95    y[ot][jt];  a96..a191 xb[ks][jt] = {h, l} (B operand of q / k stages, A operand of the v stage)"""
from h3_asm_common import ar, clobber_regs, vr, weave as _weave

STAGE, TILES = 9216, 8192
H3D_INB = 656              # float offset of in_proj bias [384] in the layer's side block; sc_in at 640
SLOT = lambda p, part: 8 * p + (0 if part == "h" else 4)
OB = lambda jt, part: 168 + 8 * jt + (0 if part == "h" else 4)
S_OFF, S_REL, S_W2048, S_STRIDE, S_AUXOFF, S_END, S_PAIR = 84, 85, 86, 88, 90, 92, 93
S_SCIN, S_SCQ, S_LOG2E, S_MASKED = 94, 95, 96, 97


def mfma32(d, a, b, zero=False, dcls="v", acls="v", bcls="v"):
    R = lambda c, x: ar(x) if c == "a" else vr(x)
    return f"v_mfma_f32_16x16x32_f16 {R(dcls, d)}, {R(acls, a)}, {R(bcls, b)}, {'0' if zero else R(dcls, d)}"


def mfma16(d, a, b, zero=False):
    return f"v_mfma_f32_16x16x16_f16 {vr(d)}, {vr(a, 2)}, {vr(b, 2)}, {'0' if zero else vr(d)}"


def weave(mfmas, valu, misc, valu_per=2, misc_per=3, skip=0):
    return _weave(mfmas, valu, misc, valu_per, misc_per, skip)


def split_pair(src, dst_h, dst_l, t):
    """4 fp32 values src..src+3 -> 2 registers of fp16 hi at dst_h, 2 of lo at dst_l (t: 4 temporaries): 8 VALU ops."""
    ops = [f"v_cvt_pk_f16_f32 v{dst_h}, v{src}, v{src + 1}", f"v_cvt_pk_f16_f32 v{dst_h + 1}, v{src + 2}, v{src + 3}"]
    for r in range(4):
        sel = "op_sel:[1,0,0] " if r % 2 else ""
        ops.append(f"v_fma_mix_f32 v{t + r}, v{dst_h + r // 2}, -1.0, v{src + r} {sel}op_sel_hi:[1,0,0]")
    ops += [f"v_cvt_pk_f16_f32 v{dst_l}, v{t}, v{t + 1}", f"v_cvt_pk_f16_f32 v{dst_l + 1}, v{t + 2}, v{t + 3}"]
    return ops


class DenseAttnStatement:
    """One dense-softmax attention statement.  Options:
    nt4     (r06; a file of its own only inside the encoder-stack statement) 64-token waves - ONE molecule of 49-64 atoms per wave
            (csrc H3N4_*), a ring of three stage buffers.  Keys = 64 = two K = 32 groups (no K = 16 tail).  What does not fit as it stands is the score tile: 4 query tiles x 4
            key tiles x 4 registers beside y (a0..a127) and the split activations (a128..a255) - so a head runs in two QUERY
            HALVES (tiles 0, 1 then 2, 3) over 32 score registers:
              V(h) | S(A) | Q(h+1) + softmax(A) | P.V(A) | S(B) | K(h+1) + softmax(B) | P.V(B) | [out_proj after an odd h]
            Register map:  v0..v31 tile slots;  v32..v79 QA KA VA[jt] (the P.V accumulators take VA's registers: v is split into
            operands before the first P.V of the head);  v80..v111 QH QL KH KL[jt];  v112..v127 VH01 VL01 VH23 VL23;
            v128..v159 SC[jl][mt] of the half in flight (P operands written over them: PL01 PL23 PH01 PH23);  v160..v164 1 / sum,
            reduction copy;  v168..v199 OB[jt];  v200..v211 temporaries;  v212..v220 biases;  v221..v229 addresses;  a0..a127 y;
            a128..a255 xb.  Key masks: ONE pair of words (%[m0l], %[m0h]: keys 0-31, 32-63 of the wave's molecule, shifted by
            the lane group) serves all four query tiles.
    fused   the block embedded in the asm statement of the whole encoder stack (gen_h3_enc_asm.py dense): the split activations
            are already in a96..a191 (written there by the glue, no trip through the LDS), the accumulators arrive holding the
            residual (x / s_o) instead of zeros, and y stays in a0..a95.
    sl      LDS address of the layer's side block (the encoder-stack statement double-buffers it: an SGPR there)
    experiment  flags of H3_ATTN_EXPERIMENT (timing only: results become wrong)."""
    WHAT, HEADER_TAIL = "dense-softmax attention", "."

    def __init__(self, nt4=False, fused=False, sl="%[sl]", experiment=()):
        self.NT4, self.FUSED, self.SL = nt4, fused, sl
        self.EXPERIMENT = frozenset(experiment)
        self.NT = 4 if nt4 else 3
        self.AHEAD = self.RING = 3 if nt4 else 5
        part = lambda p: 0 if p == "h" else 4
        if nt4:
            self.QA = lambda jt: 32 + 4 * jt
            self.KA = lambda jt: 48 + 4 * jt
            self.VA = lambda jt: 64 + 4 * jt
            self.QH = lambda jt: 80 + 2 * jt
            self.QL = lambda jt: 88 + 2 * jt
            self.KH = lambda jt: 96 + 2 * jt
            self.KL = lambda jt: 104 + 2 * jt
            self.VH01, self.VL01, self.VH23, self.VL23 = 112, 116, 120, 124
            self.SC = lambda jt, mt: 128 + 16 * (jt % 2) + 4 * mt          # the half in flight: query tiles jt % 2
            self.PL01 = lambda jt: 128 + 16 * (jt % 2)
            self.PL23 = lambda jt: 132 + 16 * (jt % 2)
            self.PH01 = lambda jt: 136 + 16 * (jt % 2)
            self.PH23 = lambda jt: 140 + 16 * (jt % 2)
            self.RS = lambda jt: 160 + jt
            self.V_RED = 164
            self.O32 = lambda jt: 64 + 4 * jt                              # P.V accumulators: v's registers (dead after prep_v)
            self.V_T = 200
            self.V_BQ, self.V_BK, self.V_BV = 212, 216, 220
            self.V_TILE, self.V_LANE16, self.V_SLQ, self.V_SLV, self.V_GN, self.V_TMP = 221, 222, 223, 224, 226, 228
            # (N_V: this block's own registers; the operand pair in v232.. / v240.. belongs to the caller's map)
            self.N_V, self.N_A = 230, 248
            self.YACC = lambda ot, jt: 4 * (4 * ot + jt)
            # the split activations: a128..a247, and the LAST operand pair (k-step 3, token tile 3) in VGPRs v232..v235 / v240..v243 -
            # registers nothing touches between the glue's operand pass and the end of this block - so that a248..a255 stay free in
            # every statement of the kernel: hipcc parks what it carries through the prologue there; with all 256 AGPRs taken it
            # went to scratch
            self.XB = lambda ks, jt, p: ((232 if p == "h" else 240) if (ks, jt) == (3, 3) else 128 + 8 * (4 * ks + jt) + part(p))
            self.XB_CLS = lambda ks, jt: "v" if (ks, jt) == (3, 3) else "a"
        else:
            self.QA = lambda jt: 32 + 4 * jt
            self.KA = lambda jt: 44 + 4 * jt
            self.VA = lambda jt: 56 + 4 * jt
            self.QH = lambda jt: 68 + 2 * jt
            self.QL = lambda jt: 74 + 2 * jt
            self.KH = lambda jt: 80 + 2 * jt
            self.KL = lambda jt: 86 + 2 * jt
            self.VH01, self.VL01, self.VH2, self.VL2 = 92, 96, 100, 102
            self.SC = lambda jt, mt: 104 + 12 * jt + 4 * mt
            self.PL01 = lambda jt: 104 + 12 * jt
            self.PH01 = lambda jt: 108 + 12 * jt
            self.PL2 = lambda jt: 112 + 12 * jt
            self.PH2 = lambda jt: 114 + 12 * jt
            self.RS = lambda jt: 140 + jt
            self.V_RED = 143                # second copy for the cross-lane reductions
            self.O32 = lambda jt: 144 + 4 * jt
            self.O16 = lambda jt: 156 + 4 * jt
            self.V_T = 192                  # v192..v203
            self.V_BQ, self.V_BK, self.V_BV = 204, 208, 203   # BV shares the last temporary slot's neighbour (v203 is never used as a temporary)
            self.V_TILE, self.V_LANE16, self.V_SLQ, self.V_SLV, self.V_GN, self.V_TMP = 212, 213, 214, 215, 216, 218
            self.N_V, self.N_A = 220, 192
            self.YACC = lambda ot, jt: 4 * (3 * ot + jt)
            self.XB = lambda ks, jt, p: 96 + 8 * (3 * ks + jt) + part(p)
            self.XB_CLS = lambda ks, jt: "a"

    def clobbers(self):
        return clobber_regs(self.N_V, self.N_A, 84, 98)

    def tile_reads(self, pair):
        return [f"ds_read_b128 {vr(SLOT(pair, 'h'))}, v{self.V_TILE} offset:{2048 * pair}",
                f"ds_read_b128 {vr(SLOT(pair, 'l'))}, v{self.V_TILE} offset:{2048 * pair + 1024}"]

    def handoff(self, next_reads, label, aux):
        V_GN, V_TMP = self.V_GN, self.V_TMP
        h = [
            f"s_mov_b32 s{S_REL}, s{S_OFF}",
            f"s_add_u32 s{S_OFF}, s{S_OFF}, {STAGE}",
            [f"s_cmp_eq_u32 s{S_OFF}, s{S_END}", f"s_cselect_b32 s{S_OFF}, %[ring], s{S_OFF}"],
        ]
        if next_reads:
            h += [f"v_add_u32 v{self.V_TILE}, s{S_OFF}, v{self.V_LANE16}"] + self.tile_reads(0) + self.tile_reads(1)
        h += [
            f"s_add_u32 m0, s{S_REL}, s{S_W2048}",
            "s_nop 0",
            f"global_load_lds_dwordx4 {vr(V_GN, 2)}, off",
            f"global_load_lds_dwordx4 {vr(V_GN, 2)}, off offset:1024",
        ]
        if aux:
            # the last five hand-offs of the section fetch the FFN's first stages, whose A0 stages carry a bias / scale block:
            # wave 0 moves it in every hand-off of the last head pair (harmless where the stage has none)
            h += [["s_cmp_lg_u32 %[wave], 0",
                   f"s_cbranch_scc1 .Lh3atd_noaux_{label}_%=",
                   f"s_cmp_lg_u32 s{S_PAIR}, 1",
                   f"s_cbranch_scc1 .Lh3atd_noaux_{label}_%=",
                   f"v_lshl_add_u64 {vr(V_TMP, 2)}, {vr(V_GN, 2)}, 0, s[{S_AUXOFF}:{S_AUXOFF + 1}]",
                   f"s_add_u32 m0, s{S_REL}, {TILES}",
                   "s_nop 0",
                   f"global_load_lds_dwordx4 {vr(V_TMP, 2)}, off",
                   f".Lh3atd_noaux_{label}_%=:"]]
        h += [f"v_lshl_add_u64 {vr(V_GN, 2)}, {vr(V_GN, 2)}, 0, s[{S_STRIDE}:{S_STRIDE + 1}]"]
        if "nodma" in self.EXPERIMENT:  # timing experiment (results wrong): no weight DMA inside the section
            h = [x for x in h if isinstance(x, str) and not x.startswith("global_load_lds")]
        return h

    def stage(self, groups, valu, label, next_reads=True, aux=True, skip=0, pre_barrier=(), valu_per=2):
        """One 4-pair weight stage: `groups[p]` = the MFMAs of tile pair p; `valu` is woven under them; `pre_barrier`: LDS reads
        issued in the second pair's shadow (they have returned by the lgkmcnt(0) in front of the barrier)."""
        valu = list(valu)
        share = -(-len(valu) // 4)
        parts = [valu[i * share:(i + 1) * share] for i in range(4)]
        out = ["s_waitcnt lgkmcnt(2)"]
        out += weave(groups[0], parts[0], self.tile_reads(2), skip=skip, valu_per=valu_per)
        out.append("s_waitcnt lgkmcnt(2)")
        out += weave(groups[1], parts[1], self.tile_reads(3) + list(pre_barrier), valu_per=valu_per)
        out.append(f"s_waitcnt vmcnt({2 * (self.AHEAD - 2)}) lgkmcnt(0)")   # stages s + 2 .. s + AHEAD - 1 may stay in flight, two DMAs each
        if "nobarrier" not in self.EXPERIMENT:
            out.append("s_barrier")
        out += weave(groups[2], parts[2], self.handoff(next_reads, label, aux), valu_per=valu_per)
        out += weave(groups[3], parts[3], [], valu_per=valu_per)
        return out

    def qk_groups(self, acc):
        """q_h / k_h stage: pair p = k-step; acc[jt] += tile(p) . xb[p][jt]  (3-term split)."""
        groups = []
        for ks in range(4):
            g = []
            for k, (ap, bp) in enumerate((("h", "h"), ("h", "l"), ("l", "h"))):
                for jt in range(self.NT):
                    g.append(mfma32(acc(jt), SLOT(ks, ap), self.XB(ks, jt, bp), zero=(ks == 0 and k == 0), bcls=self.XB_CLS(ks, jt)))
            groups.append(g)
        return groups

    def v_groups(self):
        """v_h stage, operands swapped: VA[jt] += xb[p][jt] . tile(p)  ->  [token][feature]."""
        groups = []
        for ks in range(4):
            g = []
            for k, (xp, wp) in enumerate((("h", "h"), ("l", "h"), ("h", "l"))):
                for jt in range(self.NT):
                    g.append(mfma32(self.VA(jt), self.XB(ks, jt, xp), SLOT(ks, wp), zero=(ks == 0 and k == 0), acls=self.XB_CLS(ks, jt)))
            groups.append(g)
        return groups

    def out_groups(self, half):
        groups = []
        for p in range(4):
            g = []
            for ap, bp in (("h", "h"), ("h", "l"), ("l", "h")):
                for jt in range(self.NT):
                    g.append(mfma32(self.YACC(4 * half + p, jt), SLOT(p, ap), OB(jt, bp), dcls="a"))
            groups.append(g)
        return groups

    def prep_qk(self):
        """(QA * sc/4 + bq/4) -> QH / QL, (KA * sc + bk) -> KH / KL."""
        QA, KA, V_T = self.QA, self.KA, self.V_T
        ops = []
        for jt in range(self.NT):
            t = V_T + 4 * (jt % 2)
            ops += [f"v_fma_f32 v{QA(jt) + r}, v{QA(jt) + r}, s{S_SCQ}, v{self.V_BQ + r}" for r in range(4)]
            ops += split_pair(QA(jt), self.QH(jt), self.QL(jt), t)
        for jt in range(self.NT):
            t = V_T + 4 * (jt % 2)
            ops += [f"v_fma_f32 v{KA(jt) + r}, v{KA(jt) + r}, s{S_SCIN}, v{self.V_BK + r}" for r in range(4)]
            ops += split_pair(KA(jt), self.KH(jt), self.KL(jt), t)
        return ops

    def prep_v(self):
        VA, VH01, VL01, V_T = self.VA, self.VH01, self.VL01, self.V_T
        ops = []
        for jt in range(self.NT):
            ops += [f"v_fma_f32 v{VA(jt) + r}, v{VA(jt) + r}, s{S_SCIN}, v{self.V_BV}" for r in range(4)]
        ops += split_pair(VA(0), VH01, VL01, V_T) + split_pair(VA(1), VH01 + 2, VL01 + 2, V_T + 4)
        if self.NT4:
            return ops + split_pair(VA(2), self.VH23, self.VL23, V_T) + split_pair(VA(3), self.VH23 + 2, self.VL23 + 2, V_T + 4)
        ops += split_pair(VA(2), self.VH2, self.VL2, V_T)
        return ops

    def s_mfmas(self, half=None):
        """S^T[key tile mt][query tile jt] = k_h[mt] q_h[jt]^T (K = 16, three terms).  half (64-token build): query tiles 2 half, 2 half + 1."""
        out = []
        for jt in (range(self.NT) if half is None else (2 * half, 2 * half + 1)):
            for k, (kp, qp) in enumerate(((self.KH, self.QH), (self.KH, self.QL), (self.KL, self.QH))):
                for mt in range(self.NT):
                    out.append(mfma16(self.SC(jt, mt), kp(mt), qp(jt), zero=(k == 0)))
        return out

    def reduce4(self, op, v):
        """v <- op over the four lanes sharing (lane & 15), through V_RED (v_permlane16_swap / v_permlane32_swap)."""
        V_RED = self.V_RED
        return [f"v_mov_b32 v{V_RED}, v{v}", "s_nop 1", f"v_permlane16_swap_b32 v{v}, v{V_RED}", f"{op} v{v}, v{v}, v{V_RED}",
                f"v_mov_b32 v{V_RED}, v{v}", "s_nop 1", f"v_permlane32_swap_b32 v{v}, v{V_RED}", f"{op} v{v}, v{v}, v{V_RED}"]

    def soft(self, jt):
        """Masked softmax of query tile jt over its 12 accumulator elements (keys 16 mt + 4 g + r) and the split of P,
        unnormalised (1 / sum goes to RS[jt]).  Mask bits: %[mNl] bit r (mt 0), bit 16 + r (mt 1); %[mNh] bit r (mt 2)."""
        SC, V_T, PL01, PH01, PL2, PH2 = self.SC, self.V_T, self.PL01, self.PH01, self.PL2, self.PH2
        el = [(mt, r) for mt in range(self.NT) for r in range(4)]
        m, mx, sm = V_T + 8, V_T + 9, V_T + 10
        ops = []
        for i, (mt, r) in enumerate(el):
            word, bit = (f"%[m{jt}l]", 16 * mt + r) if mt < 2 else (f"%[m{jt}h]", r)
            ops += [f"v_bfe_i32 v{m}, {word}, {bit}, 1", f"v_bfi_b32 v{SC(jt, mt) + r}, v{m}, v{SC(jt, mt) + r}, s{S_MASKED}"]
            ops.append(f"v_mov_b32 v{mx}, v{SC(jt, mt) + r}" if i == 0 else f"v_max_f32 v{mx}, v{mx}, v{SC(jt, mt) + r}")
        ops += self.reduce4("v_max_f32", mx)
        ops.append(f"v_mul_f32 v{mx}, s{S_LOG2E}, v{mx}")
        for i, (mt, r) in enumerate(el):
            x = SC(jt, mt) + r
            ops += [f"v_fma_f32 v{x}, v{x}, s{S_LOG2E}, -v{mx}", f"v_exp_f32 v{x}, v{x}"]
        for i, (mt, r) in enumerate(el):   # sums after all exps: a transcendental's result is not read by the very next op
            x = SC(jt, mt) + r
            ops.append(f"v_mov_b32 v{sm}, v{x}" if i == 0 else f"v_add_f32 v{sm}, v{sm}, v{x}")
        ops += self.reduce4("v_add_f32", sm)
        ops.append(f"v_rcp_f32 v{self.RS(jt)}, v{sm}")
        # split, in place: hi packs to temporaries, residuals in place, lo packs over the low registers, hi packs moved behind
        t = V_T
        base = SC(jt, 0)
        for k in range(4):
            ops.append(f"v_cvt_pk_f16_f32 v{t + k}, v{base + 2 * k}, v{base + 2 * k + 1}")
        for k in range(8):
            sel = "op_sel:[1,0,0] " if k % 2 else ""
            ops.append(f"v_fma_mix_f32 v{base + k}, v{t + k // 2}, -1.0, v{base + k} {sel}op_sel_hi:[1,0,0]")
        for k in range(4):
            ops.append(f"v_cvt_pk_f16_f32 v{PL01(jt) + k}, v{base + 2 * k}, v{base + 2 * k + 1}")
        for k in range(4):
            ops.append(f"v_mov_b32 v{PH01(jt) + k}, v{t + k}")
        b2 = SC(jt, 2)
        for k in range(2):
            ops.append(f"v_cvt_pk_f16_f32 v{t + 4 + k}, v{b2 + 2 * k}, v{b2 + 2 * k + 1}")
        for k in range(4):
            sel = "op_sel:[1,0,0] " if k % 2 else ""
            ops.append(f"v_fma_mix_f32 v{b2 + k}, v{t + 4 + k // 2}, -1.0, v{b2 + k} {sel}op_sel_hi:[1,0,0]")
        for k in range(2):
            ops.append(f"v_cvt_pk_f16_f32 v{PL2(jt) + k}, v{b2 + 2 * k}, v{b2 + 2 * k + 1}")
        for k in range(2):
            ops.append(f"v_mov_b32 v{PH2(jt) + k}, v{t + 4 + k}")
        return ops

    def pv_mfmas(self, jt):
        O32, O16, VH01, VL01, VH2, VL2 = self.O32, self.O16, self.VH01, self.VL01, self.VH2, self.VL2
        PH01, PL01, PH2, PL2 = self.PH01, self.PL01, self.PH2, self.PL2
        return [mfma32(O32(jt), VH01, PH01(jt), zero=True), mfma16(O16(jt), VH2, PH2(jt), zero=True),
                mfma32(O32(jt), VH01, PL01(jt)), mfma16(O16(jt), VH2, PL2(jt)),
                mfma32(O32(jt), VL01, PH01(jt)), mfma16(O16(jt), VL2, PH2(jt))]

    def osplit(self, jt, hh):
        """(O32 + O16) / sum -> elements 4 hh .. 4 hh + 3 of OB[jt].h / .l (registers + 2 hh, + 2 hh + 1)."""
        O32, O16 = self.O32, self.O16
        t = self.V_T + 4 * (jt % 2)
        ops = [f"v_add_f32 v{O32(jt) + r}, v{O32(jt) + r}, v{O16(jt) + r}" for r in range(4)]
        ops += [f"v_mul_f32 v{O32(jt) + r}, v{O32(jt) + r}, v{self.RS(jt)}" for r in range(4)]
        ops += split_pair(O32(jt), OB(jt, "h") + 2 * hh, OB(jt, "l") + 2 * hh, t)
        return ops

    def soft4(self, jt):
        """64-token build: masked softmax of query tile jt over its 16 accumulator elements (keys 16 mt + 4 g + r) and the split of P,
        unnormalised (1 / sum goes to RS[jt]).  Mask bits: %[m0l] bit 16 (mt % 2) + r for mt 0, 1; %[m0h] the same for mt 2, 3.
        P operands, in place over the 16 score registers: PL01 (+0) PL23 (+4) PH01 (+8) PH23 (+12)."""
        SC, V_T = self.SC, self.V_T
        el = [(mt, r) for mt in range(self.NT) for r in range(4)]
        m, mx, sm = V_T + 8, V_T + 9, V_T + 10
        ops = []
        for i, (mt, r) in enumerate(el):
            word, bit = ("%[m0l]" if mt < 2 else "%[m0h]"), 16 * (mt % 2) + r
            ops += [f"v_bfe_i32 v{m}, {word}, {bit}, 1", f"v_bfi_b32 v{SC(jt, mt) + r}, v{m}, v{SC(jt, mt) + r}, s{S_MASKED}"]
            ops.append(f"v_mov_b32 v{mx}, v{SC(jt, mt) + r}" if i == 0 else f"v_max_f32 v{mx}, v{mx}, v{SC(jt, mt) + r}")
        ops += self.reduce4("v_max_f32", mx)
        ops.append(f"v_mul_f32 v{mx}, s{S_LOG2E}, v{mx}")
        for mt, r in el:
            x = SC(jt, mt) + r
            ops += [f"v_fma_f32 v{x}, v{x}, s{S_LOG2E}, -v{mx}", f"v_exp_f32 v{x}, v{x}"]
        for i, (mt, r) in enumerate(el):
            x = SC(jt, mt) + r
            ops.append(f"v_mov_b32 v{sm}, v{x}" if i == 0 else f"v_add_f32 v{sm}, v{sm}, v{x}")
        ops += self.reduce4("v_add_f32", sm)
        ops.append(f"v_rcp_f32 v{self.RS(jt)}, v{sm}")
        # split, in place: the eight hi packs to temporaries, the sixteen residuals in place, lo packs over registers 0..7, hi packs to 8..15
        t, base = V_T, SC(jt, 0)
        for k in range(8):
            ops.append(f"v_cvt_pk_f16_f32 v{t + k}, v{base + 2 * k}, v{base + 2 * k + 1}")
        for k in range(16):
            sel = "op_sel:[1,0,0] " if k % 2 else ""
            ops.append(f"v_fma_mix_f32 v{base + k}, v{t + k // 2}, -1.0, v{base + k} {sel}op_sel_hi:[1,0,0]")
        for k in range(8):
            ops.append(f"v_cvt_pk_f16_f32 v{self.PL01(jt) + k}, v{base + 2 * k}, v{base + 2 * k + 1}")
        for k in range(8):
            ops.append(f"v_mov_b32 v{self.PH01(jt) + k}, v{t + k}")
        return ops

    def pv4_mfmas(self, half):
        """O^T[feature][query] of query tiles 2 half, 2 half + 1: one chain of six K = 32 MFMAs per tile (keys 0-31, 32-63 x three
        terms), the two chains interleaved."""
        O32, VH01, VL01, VH23, VL23 = self.O32, self.VH01, self.VL01, self.VH23, self.VL23
        PH01, PL01, PH23, PL23 = self.PH01, self.PL01, self.PH23, self.PL23
        chains = []
        for jt in (2 * half, 2 * half + 1):
            chains.append([mfma32(O32(jt), VH01, PH01(jt), zero=True), mfma32(O32(jt), VH23, PH23(jt)),
                           mfma32(O32(jt), VH01, PL01(jt)), mfma32(O32(jt), VH23, PL23(jt)),
                           mfma32(O32(jt), VL01, PH01(jt)), mfma32(O32(jt), VL23, PH23(jt))])
        return [m for pair in zip(*chains) for m in pair]

    def osplit4(self, jt, hh):
        """O / sum -> elements 4 hh .. 4 hh + 3 of OB[jt].h / .l."""
        O32 = self.O32
        t = self.V_T + 4 * (jt % 2)
        ops = [f"v_mul_f32 v{O32(jt) + r}, v{O32(jt) + r}, v{self.RS(jt)}" for r in range(4)]
        return ops + split_pair(O32(jt), OB(jt, "h") + 2 * hh, OB(jt, "l") + 2 * hh, t)

    def head_slot4(self, hh, L):
        """One head of the 64-token build (see the nt4 note at the top)."""
        A = L.append
        tag = f"h{hh}"
        bq4 = [f"v_mul_f32 v{self.V_BQ + r}, 0.25, v{self.V_BQ + r}" for r in range(4)]
        # ---- stage V(h) | q, k of this head: scale, bias, split (their biases were read in the K stage before)
        L += self.stage(self.v_groups(), bq4 + self.prep_qk(), f"{tag}v", skip=1)
        for half, nxt in ((0, self.QA), (1, self.KA)):
            # ---- S(half) | half 0: v of this head (scale, bias, split); half 1: 1 / sum and split of O for the first two query tiles
            A("s_nop 3")
            L += weave(self.s_mfmas(half), self.prep_v() if half == 0 else self.osplit4(0, hh) + self.osplit4(1, hh), [],
                       skip=3 if half == 0 else 8, valu_per=2)
            # ---- stage Q(h+1) / K(h+1) | masked softmax + split of P of this half (bare after the last head)
            sv = self.soft4(2 * half) + self.soft4(2 * half + 1)
            if hh == 1:
                A(f"s_cmp_eq_u32 s{S_PAIR}, 1")
                A(f"s_cbranch_scc1 .Lh3atd_last{half}_{tag}_%=")
            L += self.stage(self.qk_groups(nxt), sv, f"{tag}{'qk'[half]}", skip=3, pre_barrier=self.bias_reads() if half == 1 else (),
                            valu_per=3)
            if hh == 1:
                A(f"s_branch .Lh3atd_pv{half}_{tag}_%=")
                A(f".Lh3atd_last{half}_{tag}_%=:")
                A("s_nop 7")
                L += sv
                A(f".Lh3atd_pv{half}_{tag}_%=:")
            # ---- P.V of this half (the accumulators are v's: dead since prep_v)
            A("s_nop 3")
            L += self.pv4_mfmas(half)
        A("s_nop 15")    # (the last P.V MFMAs are eight passes each: their results are read next)
        A("s_nop 15")
        A("s_nop 15")
        L += self.osplit4(2, hh)
        L += self.osplit4(3, hh)
        # ---- out_proj k-step of the pair
        if hh == 1:
            A("s_nop 7")
            L += self.stage(self.out_groups(0), [], f"{tag}oa")
            L += self.stage(self.out_groups(1), [], f"{tag}ob")

    def bias_reads(self):
        """q / k / v bias of the head at V_SLQ / V_SLV (advanced afterwards); q's is pre-multiplied by 1/4 by the caller."""
        V_SLQ, V_SLV = self.V_SLQ, self.V_SLV
        return [f"ds_read_b128 {vr(self.V_BQ)}, v{V_SLQ} offset:{4 * H3D_INB}",
                f"ds_read_b128 {vr(self.V_BK)}, v{V_SLQ} offset:{4 * (H3D_INB + 128)}",
                f"ds_read_b32 v{self.V_BV}, v{V_SLV} offset:{4 * (H3D_INB + 256)}",
                f"v_add_u32 v{V_SLQ}, 64, v{V_SLQ}",
                f"v_add_u32 v{V_SLV}, 64, v{V_SLV}"]

    def head_slot(self, hh, L):
        EXPERIMENT = self.EXPERIMENT
        A = L.append
        tag = f"h{hh}"
        # ---- A: stage V(h) | q, k of this head: scale, bias, split.  The head's biases were read in the K stage before.
        bq4 = [f"v_mul_f32 v{self.V_BQ + r}, 0.25, v{self.V_BQ + r}" for r in range(4)]
        noprep = "noprep" in EXPERIMENT
        L += self.stage(self.v_groups(), [] if noprep else bq4 + self.prep_qk(), f"{tag}v", skip=1)
        # ---- B: S(h) | v of this head
        A("s_nop 3")
        L += weave([] if "nos" in EXPERIMENT else self.s_mfmas(), [] if noprep else self.prep_v(), [], skip=3)
        # ---- C: stages Q(h+1), K(h+1) | softmax + split of P(h)
        sv = [] if "nosoft" in EXPERIMENT else self.soft(0) + self.soft(1) + self.soft(2)   # (timing experiments: results wrong)
        half = len(sv) // 2
        if hh == 1:
            A(f"s_cmp_eq_u32 s{S_PAIR}, 1")
            A(f"s_cbranch_scc1 .Lh3atd_last_{tag}_%=")
        L += self.stage(self.qk_groups(self.QA), sv[:half], f"{tag}q", skip=3, valu_per=3)
        L += self.stage(self.qk_groups(self.KA), sv[half:], f"{tag}k", skip=0, pre_barrier=self.bias_reads(), valu_per=3)
        if hh == 1:
            A(f"s_branch .Lh3atd_pv_{tag}_%=")
            A(f".Lh3atd_last_{tag}_%=:")
            A("s_nop 7")
            L += sv                      # after the last head there is nothing left to hide it under
            A(f".Lh3atd_pv_{tag}_%=:")
        # ---- D: P.V(h) | 1 / sum and split of O for the tiles already done
        A("s_nop 3")
        if "nopv" not in EXPERIMENT:
            L += self.pv_mfmas(0) + self.pv_mfmas(1)
            L += weave(self.pv_mfmas(2), self.osplit(0, hh), [], skip=1)
            A("s_nop 7")
            L += self.osplit(1, hh)
            A("s_nop 7")
            L += self.osplit(2, hh)
        # ---- E: out_proj k-step of the pair
        if hh == 1:
            A("s_nop 7")
            L += self.stage(self.out_groups(0), [], f"{tag}oa")
            L += self.stage(self.out_groups(1), [], f"{tag}ob")

    def generate(self):
        NT, FUSED, SL, XB, XB_CLS = self.NT, self.FUSED, self.SL, self.XB, self.XB_CLS
        V_T, V_TILE, V_LANE16, V_SLQ, V_SLV, V_GN, V_TMP = \
            self.V_T, self.V_TILE, self.V_LANE16, self.V_SLQ, self.V_SLV, self.V_GN, self.V_TMP
        L = []
        A = L.append
        A(f"v_mbcnt_lo_u32_b32 v{V_LANE16}, -1, 0")
        A(f"v_mbcnt_hi_u32_b32 v{V_LANE16}, -1, v{V_LANE16}")
        # side-block lane addresses: f4 at feature 4 g (q, k biases), float at feature (lane & 15) (v bias)
        A(f"v_lshrrev_b32 v{V_T}, 4, v{V_LANE16}")
        A(f"v_lshlrev_b32 v{V_T}, 4, v{V_T}")
        A(f"v_add_u32 v{V_SLQ}, {SL}, v{V_T}")
        A(f"v_and_b32 v{V_T}, 15, v{V_LANE16}")
        A(f"v_lshlrev_b32 v{V_T}, 2, v{V_T}")
        A(f"v_add_u32 v{V_SLV}, {SL}, v{V_T}")
        A(f"v_lshlrev_b32 v{V_LANE16}, 4, v{V_LANE16}")
        A(f"s_lshl_b32 s{S_W2048}, %[wave], 11")
        A(f"s_mov_b32 s{S_W2048 + 1}, 0")
        A(f"s_mov_b32 s{S_STRIDE}, {STAGE}")
        A(f"s_mov_b32 s{S_STRIDE + 1}, 0")
        A(f"s_mov_b32 s{S_AUXOFF}, {TILES}")
        A(f"s_mov_b32 s{S_AUXOFF + 1}, 0")
        A(f"s_mov_b32 s{S_LOG2E}, 0x3fb8aa3b")
        A(f"s_mov_b32 s{S_MASKED}, 0xc6ea6000")          # -3e4
        A(f"s_add_u32 s{S_END}, %[ring], {self.RING * STAGE}")
        A(f"v_lshl_add_u64 {vr(V_GN, 2)}, %[gn], 0, s[{S_W2048}:{S_W2048 + 1}]")
        A(f"s_mul_i32 s{S_OFF}, %[cur], {STAGE}")
        A(f"s_add_u32 s{S_OFF}, s{S_OFF}, %[ring]")
        A(f"v_add_u32 v{V_TILE}, s{S_OFF}, v{V_LANE16}")
        # in_proj scale (side block slot 640) -> SGPRs (and a quarter of it for q).  Per-section build: the layer's side block was
        # requested by wave 0 only a few hundred cycles ago and nothing has waited for that DMA yet - the read sits behind the two
        # bare prologue stages below (two hand-offs: vmcnt wait + barrier; the first use of the scale is in the stage after them).
        # Encoder-stack build: the block arrived a whole layer ago (double-buffered), so the read can be the first thing.
        def read_scale():
            A(f"v_mov_b32 v{V_T}, {SL}")
            A(f"ds_read_b32 v{V_T + 1}, v{V_T} offset:{4 * 640}")

        def scale_to_sgprs():
            A(f"v_mul_f32 v{V_T + 2}, 0.25, v{V_T + 1}")
            A("s_nop 1")
            A(f"v_readfirstlane_b32 s{S_SCIN}, v{V_T + 1}")
            A(f"v_readfirstlane_b32 s{S_SCQ}, v{V_T + 2}")

        if FUSED:
            read_scale()
        if not FUSED:
            # split activations from the wave-private block: 24 images -> a96..a191
            A(f"v_add_u32 v{V_TMP}, %[priv], v{V_LANE16}")
            for i in range(8 * NT):
                ks, jt, part = i // (2 * NT), (i // 2) % NT, "hl"[i % 2]
                dst = (vr if XB_CLS(ks, jt) == "v" else ar)(XB(ks, jt, part))
                A(f"ds_read_b128 {dst}, v{V_TMP} offset:{1024 * i}")
            for i in range(32 * NT):
                A(f"v_accvgpr_write_b32 a{i}, 0")
        A("s_waitcnt lgkmcnt(0)")
        if FUSED:
            scale_to_sgprs()
        for r in self.tile_reads(0) + self.tile_reads(1):
            A(r)
        # ---- prologue: stages Q(0), K(0) bare; biases of head 0
        L += self.stage(self.qk_groups(self.QA), [], "pq", aux=False)
        if FUSED:
            L += self.stage(self.qk_groups(self.KA), [], "pk", aux=False, pre_barrier=self.bias_reads())
        else:
            # (the head's biases come from the same side block: read behind both hand-offs as well)
            L += self.stage(self.qk_groups(self.KA), [], "pk", aux=False)
            read_scale()
            L += self.bias_reads()
            A("s_waitcnt lgkmcnt(0)")   # LDS reads return in order: the next stage's four tile reads (older) land with them
            scale_to_sgprs()
        A(f"s_mov_b32 s{S_PAIR}, 4")
        A(".Lh3atd_pair_%=:")
        (self.head_slot4 if self.NT4 else self.head_slot)(0, L)
        (self.head_slot4 if self.NT4 else self.head_slot)(1, L)
        A(f"s_sub_u32 s{S_PAIR}, s{S_PAIR}, 1")
        A(f"s_cmp_eq_u32 s{S_PAIR}, 0")
        A("s_cbranch_scc0 .Lh3atd_pair_%=")
        # ---- out: ring slot index, y through the wave-private block, DMA pointer
        A(f"s_sub_u32 s{S_REL}, s{S_OFF}, %[ring]")
        A("s_mov_b32 %[cur], 0")
        for k in range(1, self.RING):
            A(f"s_cmp_eq_u32 s{S_REL}, {k * STAGE}")
            A(f"s_cselect_b32 %[cur], {k}, %[cur]")
        A("s_waitcnt lgkmcnt(0)")
        A("s_nop 15")
        A("s_nop 15")
        if not FUSED:
            A(f"v_add_u32 v{V_TMP}, %[priv], v{V_LANE16}")
            for i in range(8 * NT):
                for r in range(4):
                    A(f"v_accvgpr_read_b32 v{V_T + (i % 2) * 4 + r}, a{4 * i + r}")
                A(f"ds_write_b128 v{V_TMP}, {vr(V_T + (i % 2) * 4)} offset:{1024 * i}")
            A("s_waitcnt lgkmcnt(0)")
        A(f"s_sub_u32 s{S_AUXOFF}, 0, s{S_W2048}")
        A(f"s_subb_u32 s{S_AUXOFF + 1}, 0, 0")
        A(f"v_lshl_add_u64 %[gn], {vr(V_GN, 2)}, 0, s[{S_AUXOFF}:{S_AUXOFF + 1}]")
        return L


if __name__ == "__main__":
    import h3_asm_manifest
    h3_asm_manifest.main("dense_attn")
