"""gen_t16r.py -- generator of expm_t16r_asm: expm_t16q_asm (gen_t16q.py) with the LDS instructions of its two mirrored-tile
exchanges, and the first fragment requests of every product, issued in the shadow of matrix instructions.

What it replaces: the `exp` inside ExpProp's prop_step! (/root/reference/src/optimize.jl:732), like the base kernel.

Every fp64 operation of expm_t16q_asm is here, on the same elements, in the same order per element and per accumulator: the
results are the same to the bit on every path.  What moves is LDS instructions, waits, barriers and whole groups of matrix
instructions.  What an exchange costs a wave is not the drain of its stores or its barrier but the ISSUE of its LDS instructions
in the open (~28 cycles each, gen_t16.py); moving the stores and the barrier alone gained nothing (profiles/t16r_ab.txt, "bloc").

  A2 = A A           the last k-block runs slot by slot, slot 1 first (Gen.product, tail=).  Behind slot 1's twelve matrix
  (every cell)       instructions the slots whose tiles other waves need -- slot 1 and the half slot 2 -- are complete: their
                     A2 is formed there, and the sixteen exchange stores ride behind slot 0's twelve matrix instructions, two
                     behind each of the first four, one behind each of the rest.  The s_waitcnt / s_barrier pair stands where
                     it stood.
  y0 = c1 A2 A2      the same order; slot 0's matrix instructions are split around the barrier: six in front of it with the
  (marked cells)     sixteen stores behind them, six behind it with the eight exchange reads behind them.  The conjugating adds
                     stand behind these six and fill the wait states in front of slot 0's own linear combination.  Nothing is
                     outstanding at the join in front of the third product, so the load tracker of gcn.py is what it was.
                     The reads of the FIRST exchange, which expm_t16q_asm requests in the open behind the fork, ride behind slot
                     0's matrix instructions of this product's first k-block; slot 2's linear combination consumes them behind
                     those twelve, as before.
  every product      lead_ride: of the fragment requests of the first k-step behind a barrier only plane 0's stand in the
                     open; those of the planes 1 and 2 ride behind the matrix instructions of the plane before.
  the stand-in       the marked path of expm_t16q_asm carries one matrix instruction whose result is dropped, so that 625 is
                     booked; this kernel leaves it out: 120 + 120 + 2 * 192 = 624 per marked cell and wave, like the compiled
                     twin.

Variants of a whole code object for timing (GRAPE_T16_OPTS, tools/co_ab.sh): x1late -- the first exchange as in expm_t16q_asm;
x2late -- the second; bloc -- the exchanges' LDS instructions in one piece; split2=N -- N of slot 0's last twelve matrix
instructions in front of the second barrier; nolead, noride0 -- the lead requests / the reads of the first exchange in the open;
drop -- the stand-in instruction stays (the host books 624 all the same: timing only).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gcn import S, Neg, kernel_text  # noqa: E402
from gen_t16 import E1, E2, EXH, LDS_BYTES, KERNARG  # noqa: E402
from gen_t16q import GenQ  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MFMA_R = 120 + 120 + 2 * 192
SPLIT2 = 6          # matrix instructions of slot 0 in front of the barrier of the second exchange (of its last twelve)


class GenR(GenQ):
    def __init__(self, name="expm_t16r_asm", **kw):
        super().__init__(name=name, **kw)
        self.split2 = SPLIT2
        self.lead_ride = not self.opts.get("nolead")
        for o in self.opts:             # (timing variants: split2=N)
            if o.startswith("split2="):
                self.split2 = int(o[7:])
        assert 0 <= self.split2 <= 12

    def bound_stand_in(self, A2re):
        if self.opts.get("drop"):
            super().bound_stand_in(A2re)

    def exchange_thunks(self, re1, im1, re2, im2):
        """the sixteen stores of Gen.exchange_writes, one thunk each (opts bloc: issued here, in one piece)"""
        p = self.p
        th = []
        for r in range(4):
            for addr, x, off in ((self.v_EW2, re2, 0), (self.v_EW2, im2, EXH), (self.v_EW1, re1, 0), (self.v_EW1, im1, EXH)):
                th.append(lambda addr=addr, x=x, off=off, r=r: p.ds_write(64, addr, x.d(r), off + 128 * r))
        return self.ride(th)

    def ride(self, thunks):
        if self.opts.get("bloc"):
            for f in thunks:
                f()
            return []
        return thunks

    def first_square(self, Qt, B_As, hook_store, bload_A, Uprev):
        if self.opts.get("x1late"):
            return super().first_square(Qt, B_As, hook_store, bload_A, Uprev)
        p, vp, ap = self.p, self.vp, self.ap
        # (generator bookkeeping: A2 takes the registers of the previous result, as in the base cell.  The tiles written in
        # front of slot 0's last matrix instructions -- A2re[1], A2re[2], A2im[1], A2im[2] -- held elements of the previous
        # result whose stores were issued in k-blocks 0..2 and, the last two, behind the first two k-steps of slot 1)
        vp.free(Uprev)
        A2re, A2im, A2sm = [vp.alloc() for _ in range(4)], [vp.alloc() for _ in range(4)], [vp.alloc() for _ in range(4)]
        assert A2im[2].idx == Uprev.idx + 48 and A2sm[0].idx >= Uprev.idx + Uprev.n

        def mid():
            self.a2_streams(Qt, A2re, A2im, (2, 1))
            return self.exchange_thunks(A2re[1], A2im[1], A2re[2], A2im[2])

        self.product(Qt[:3], B_As, half_last=True, hook=hook_store, bload=bload_A, tail={"mid": mid})
        ap.free(self.As_sm)
        self.stamp(1)
        self.a2_streams(Qt, A2re, A2im, (0,))
        p.s_waitcnt(lgkm=0)
        p.s_barrier()                                   # the tiles are published (also: everybody is done reading A)
        return A2re, A2im, A2sm

    def second_product_square(self, cx, L_join):
        if self.opts.get("x2late"):
            return super().second_product_square(cx, L_join)
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
        # (the reads of the first exchange ride behind slot 0's matrix instructions of the first k-block, in the gaps that carry
        # one LDS instruction or none; slot 2's linear combination, which consumes them, stands behind those twelve)
        txr, txi = vp.alloc(), vp.alloc()
        th = []
        for h in range(2):
            for dst, off in ((txr, 0), (txi, EXH), (A2re[3], E2 - E1), (A2im[3], (E2 - E1) + EXH)):
                th.append(lambda dst=dst, off=off, h=h: p.ds_read(128, dst.sub(4 * h, 4), self.v_ER, off + 16 * h))
        ride0 = []
        if self.opts.get("noride0"):
            for f in th:
                f()
        else:
            ride0 = list(zip((0, 2, 3, 4, 6, 7, 8, 10), th))
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

        kq = S(58, 2)

        def y0_in_place(slots):
            """y0 = c1 A2 A2 in place (p1 <- re, p3 <- im)"""
            self.smov64(kq, self.cq["C1"])
            streams = []
            for sl in slots:
                for r in range(4):
                    p1, p2, p3 = (Qt[sl][j].d(r) for j in range(3))
                    streams.append([lambda p3=p3, p1=p1: p.valu("v_add_f64", p3, p3, Neg(p1)),
                                    lambda p1=p1, p2=p2: p.valu("v_add_f64", p1, p1, Neg(p2)),
                                    lambda p3=p3, p2=p2: p.valu("v_add_f64", p3, p3, Neg(p2)),
                                    lambda p1=p1: p.valu("v_mul_f64", p1, kq, p1),
                                    lambda p3=p3: p.valu("v_mul_f64", p3, kq, p3)])
            for g in range(0, len(streams), 4):
                self.interleave(streams[g:g + 4])

        def mid():
            # slots 2 and 1 are complete (slot 2 first: its sums are old, slot 1's last results need their wait states)
            y0_in_place((2, 1))
            return self.exchange_thunks(Qt[1][0], Qt[1][2], Qt[2][0], Qt[2][2])

        tx2 = []

        def split():
            p.s_waitcnt(lgkm=0)
            p.s_barrier()                               # everybody is done reading the planes; the tiles are published
            xr, xi = vp.alloc(), vp.alloc()
            tx2[:] = [xr, xi]
            th = []
            for h in range(2):
                for dst, off in ((xr, 0), (xi, EXH), (Qt[3][0], E2 - E1), (Qt[3][2], (E2 - E1) + EXH)):
                    th.append(lambda dst=dst, off=off, h=h: p.ds_read(128, dst.sub(4 * h, 4), self.v_ER, off + 16 * h))
            return self.ride(th)

        # ================= A2 A2 (Hermitian square: slots 0..2, slot 2 half), the planes <- A2 inside its first k-block ======
        self.product(Qt[:3], [A2re, A2im, A2sm], half_last=True,
                     fused={"valu": valu, "stores": lambda sl: self.plane_stores(sl, A2re[sl], A2im[sl], A2sm[sl]),
                            "post": self.cell_coeffs(True), "ride0": ride0},
                     tail={"mid": mid, "split": split, "split_at": self.split2})
        for t in A2sm:
            vp.free(t)
        self.bound_stand_in(A2re)
        self.cell_bases_finish(self.s_nkc)
        self.stamp(3)
        txr, txi = tx2
        for r in range(4):
            p.valu("v_add_f64", Qt[2][0].d(r), Qt[2][0].d(r), txr.d(r))
            p.valu("v_add_f64", Qt[2][2].d(r), Qt[2][2].d(r), Neg(txi.d(r)))
        for r in range(4):
            p.valu("v_mul_f64", Qt[3][2].d(r), Qt[3][2].d(r), -1.0)
        vp.free(txr)
        vp.free(txi)
        y0_in_place((0,))
        p.salu("s_and_b32", self.s_prop, self.s_prop, 1)                 # the verdict is the plan's "ok": bit 1 stays clear
        self.stamp(4)
        assert sorted(vp.free_tiles) == sorted(joined), (vp.free_tiles, joined)
        # (the hazard tracker follows the list: what stands behind the join is spaced against this path; the other path
        # reaches the join through its own padding, gen_t16.py)


def generate(path=None, **kw):
    g = GenR(**kw)
    prog = g.build()
    text = kernel_text(prog, KERNARG, LDS_BYTES)
    if path:
        with open(path, "w") as f:
            f.write(text)
    return g, prog, text


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "expm_t16r_asm.s")
    g, prog, _ = generate(out)
    print(f"{out}: {len(prog.ins)} lines, {prog.count('mfma')} matrix instructions, {prog.count('valu') + prog.count('dpp')} vector, "
          f"{prog.count('lds')} LDS, {prog.count('vmem')} global, {prog.count('barrier')} barriers, {prog.auto_nops} wait states inserted")
