"""gen_t16q.py -- generator of expm_t16q_asm: the four-product exponential of gen_t16.py whose SECOND product is a Hermitian
square on the cells the plan of the evaluation marks (splan bit 9), Hermitian generators, shared controls, 49 <= N <= 64.

What it replaces: the `exp` inside ExpProp's prop_step! (/root/reference/src/optimize.jl:732), like the base kernel.

With c2 = 0 (coefficient set T16Q_* of grape_t18_coeffs.h, tools/t16_coeffs.py q) the second product of the scheme is

    y0 = c1 A2 A2,

the square of a Hermitian matrix: like A2 = A A it needs the upper half of the tiles only -- slots 0 and 1 of a wave's column
strip in full, slot 2 over half of the k range, slot 3 not at all: 120 matrix instructions instead of 192 -- and the mirrored
tiles come from the waves that hold them, through the exchange areas of the first product.  The price is the x^15 term of
the polynomial (structurally zero): the set is good for spectra inside 1.11, not 1.36, and which cells those are is decided
before the launch from the trace tables (t16_plan_kernel).  A walk meets both kinds of cells, so the cell has both paths
behind ONE scalar branch in front of the second product; they join in front of the third:

  bit 9 clear   the base cell, instruction for instruction (in-cell bound or certified bit 8, T16_* coefficients)
  bit 9 set     left operand: A2 itself, stored to the planes row tile by row tile inside the first k-block (the fused
                pipeline of the base class with three output slots); right operand: A2 in the vector half, as before;
                y0 <- c1 (p1 - p2, p3 - p1 - p2) on slots 0..2; second exchange (half sums of slot 2 to wave w + 2, the
                slot-1 tile to wave w + 1, which holds it as its slot 3); no bound, no verdict store (the plan wrote 0);
                one matrix instruction whose result is dropped rides under the exchange reads, so that the executed-work
                counter books 120 + 120 + 2 * 192 + 1 = 625 per cell and wave against the 697 of the other path

Products three and four are emitted once: their coefficients c3..c16 come from scalar registers, loaded per cell on either
path behind the first k-block of the second product (scalar instructions in the shadow of its matrix instructions).
Walks, squarings (a marked cell has none planned), commit and stores are the base class's.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gcn import S, Neg, kernel_text  # noqa: E402
import gen_t16 as g16  # noqa: E402
from gen_t16 import E1, E2, EXH, LDS_BYTES, KERNARG  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
Q_BIT = 0x200       # splan[cell] bit 9: the second product of this cell is the Hermitian square (t16_plan_kernel)
MFMA_Q = 120 + 120 + 2 * 192 + 1


def t16q_coeffs():
    txt = open(os.path.join(HERE, "..", "grape_t18_coeffs.h")).read()
    c = {}
    for m in re.finditer(r"#define\s+T16Q_(C\d+|THETA)\s+([-+0-9.eE]+)", txt):
        c[m.group(1)] = float(m.group(2))
    assert len(c) == 17 and c["C2"] == 0.0, c
    return c


class GenQ(g16.Gen):
    def __init__(self, name="expm_t16q_asm", **kw):
        super().__init__(name=name, **kw)
        self.cq = t16q_coeffs()

    def cell_coeffs(self, q):
        c = self.cq if q else self.c

        def load():
            for i in range(3, 16):
                self.smov64(self.s_c[i], c[f"C{i}"])
        return load

    def load_c16(self, k16):
        p = self.p
        lo, hi = g16.dbits(self.c["C16"])
        qlo, qhi = g16.dbits(self.cq["C16"])
        p.salu("s_and_b32", self.s_tmp[4], self.s_scur, Q_BIT)           # (scc: the marked cell)
        self.ssel(k16.sub(0), qlo, lo)
        self.ssel(k16.sub(1), qhi, hi)

    def second_product_fork(self, cx):
        p = self.p
        uid = len(p.ins)
        cx.L_q = f"L_q_{uid}"
        cx.pool = list(self.vp.free_tiles)
        p.salu("s_and_b32", self.s_tmp[0], self.s_scur, Q_BIT)
        p.s_branch("s_cbranch_scc1", cx.L_q)

    def bound_stand_in(self, A2re):
        # (the matrix instruction the counter books for the bound of the other path: operands whatever, result dropped)
        drop = self.vp.alloc()
        self.p.mfma(drop, A2re[0].d(0), A2re[0].d(0), 0)
        self.vp.free(drop)

    def second_product_square(self, cx, L_join):
        p, vp = self.p, self.vp
        Qt, A2re, A2im, A2sm = cx.Qt, cx.A2re, cx.A2im, cx.A2sm
        p.s_branch("s_branch", L_join)
        p.label(cx.L_q)
        # (generator bookkeeping: the register pools as they were at the fork; both paths must leave them alike)
        joined = list(vp.free_tiles)
        vp.free_tiles[:] = cx.pool

        # (the fork stands right behind the barrier of the first exchange, where nothing is outstanding: a branch waits for
        # every load in flight.  So this path requests the next cell's scalars and the exchanged tiles itself, like the other)
        self.advance()
        self.cell_bases_issue(self.s_nkc, self.s_nn, self.s_ncell)
        txr, txi = vp.alloc(), vp.alloc()
        for h in range(2):
            p.ds_read(128, txr.sub(4 * h, 4), self.v_ER, 16 * h)
            p.ds_read(128, txi.sub(4 * h, 4), self.v_ER, EXH + 16 * h)
            p.ds_read(128, A2re[3].sub(4 * h, 4), self.v_ER, (E2 - E1) + 16 * h)
            p.ds_read(128, A2im[3].sub(4 * h, 4), self.v_ER, (E2 - E1) + EXH + 16 * h)
        self.stamp(2)
        tx1 = (txr, txi)

        def valu(sl):
            if sl == 2:     # slots 2 and 3 of A2 need what the other waves sent (requested behind the barrier)
                for r in range(4):
                    p.valu("v_add_f64", A2re[2].d(r), A2re[2].d(r), tx1[0].d(r))
                    p.valu("v_add_f64", A2im[2].d(r), A2im[2].d(r), Neg(tx1[1].d(r)))
                for r in range(4):
                    p.valu("v_mul_f64", A2im[3].d(r), A2im[3].d(r), -1.0)
                vp.free(tx1[0])
                vp.free(tx1[1])
            for r in range(4):
                p.valu("v_add_f64", A2sm[sl].d(r), A2re[sl].d(r), A2im[sl].d(r))

        # ================= A2 A2 (Hermitian square: slots 0..2, slot 2 half), the planes <- A2 inside its first k-block ======
        self.product(Qt[:3], [A2re, A2im, A2sm], half_last=True,
                     fused={"valu": valu, "stores": lambda sl: self.plane_stores(sl, A2re[sl], A2im[sl], A2sm[sl]),
                            "post": self.cell_coeffs(True)})
        for t in A2sm:
            vp.free(t)
        self.cell_bases_finish(self.s_nkc)
        self.stamp(3)
        # ---- y0 = c1 A2 A2 in place on slots 0..2 (p1 <- re, p3 <- im) ----
        kq = S(58, 2)
        self.smov64(kq, self.cq["C1"])
        streams = []
        for sl in range(3):
            for r in range(4):
                p1, p2, p3 = (Qt[sl][j].d(r) for j in range(3))
                streams.append([lambda p3=p3, p1=p1: p.valu("v_add_f64", p3, p3, Neg(p1)),
                                lambda p1=p1, p2=p2: p.valu("v_add_f64", p1, p1, Neg(p2)),
                                lambda p3=p3, p2=p2: p.valu("v_add_f64", p3, p3, Neg(p2)),
                                lambda p1=p1: p.valu("v_mul_f64", p1, kq, p1),
                                lambda p3=p3: p.valu("v_mul_f64", p3, kq, p3)])
        for g in range(0, len(streams), 4):
            self.interleave(streams[g:g + 4])
        # exchange, as behind the first product: half sum of slot 2 -> wave w + 2, slot-1 tile -> wave w + 1; the reader conjugates
        for r in range(4):
            p.ds_write(64, self.v_EW2, Qt[2][0].d(r), 128 * r)
            p.ds_write(64, self.v_EW2, Qt[2][2].d(r), EXH + 128 * r)
            p.ds_write(64, self.v_EW1, Qt[1][0].d(r), 128 * r)
            p.ds_write(64, self.v_EW1, Qt[1][2].d(r), EXH + 128 * r)
        p.s_waitcnt(lgkm=0)
        p.s_barrier()                                   # everybody is done reading the planes; the tiles are published
        txr, txi = vp.alloc(), vp.alloc()
        for h in range(2):
            p.ds_read(128, txr.sub(4 * h, 4), self.v_ER, 16 * h)
            p.ds_read(128, txi.sub(4 * h, 4), self.v_ER, EXH + 16 * h)
            p.ds_read(128, Qt[3][0].sub(4 * h, 4), self.v_ER, (E2 - E1) + 16 * h)
            p.ds_read(128, Qt[3][2].sub(4 * h, 4), self.v_ER, (E2 - E1) + EXH + 16 * h)
        self.bound_stand_in(A2re)
        for r in range(4):
            p.valu("v_add_f64", Qt[2][0].d(r), Qt[2][0].d(r), txr.d(r))
            p.valu("v_add_f64", Qt[2][2].d(r), Qt[2][2].d(r), Neg(txi.d(r)))
        for r in range(4):
            p.valu("v_mul_f64", Qt[3][2].d(r), Qt[3][2].d(r), -1.0)
        vp.free(txr)
        vp.free(txi)
        p.salu("s_and_b32", self.s_prop, self.s_prop, 1)                 # the verdict is the plan's "ok": bit 1 stays clear
        self.stamp(4)
        assert sorted(vp.free_tiles) == sorted(joined), (vp.free_tiles, joined)
        # (the hazard tracker follows the list: what stands behind the join is spaced against this path; the other path
        # reaches the join through its own padding, gen_t16.py)


def generate(path=None, **kw):
    g = GenQ(**kw)
    prog = g.build()
    text = kernel_text(prog, KERNARG, LDS_BYTES)
    if path:
        with open(path, "w") as f:
            f.write(text)
    return g, prog, text


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "expm_t16q_asm.s")
    g, prog, _ = generate(out)
    print(f"{out}: {len(prog.ins)} lines, {prog.count('mfma')} matrix instructions, {prog.count('valu') + prog.count('dpp')} vector, "
          f"{prog.count('lds')} LDS, {prog.count('vmem')} global, {prog.auto_nops} wait states inserted")
