// What the last evaluation left on the device (host code only, no kernels, no HIP).
//
// StoredEval: one record per handle -- closed, open, shard -- of the facts every call that reads the stored states asks about:
// do the forward states belong to one successful forward half on the current grid, what did the backward half behind it leave,
// and has anything touched the tangent storage since the forward half of a split Hessian-vector product.  Whatever can happen
// to a handle is an event, a member function that moves all three parts at once; whoever reads the stored states asks a const
// query, which answers nullptr (go ahead) or the reason, and prefixes its own name.  Every sentence is written once, here;
// tests/evalstate_driver.cpp holds them a second time, as the table a changed word fails against.
#pragma once

#include <string>

struct StoredEval {
    enum Forward { FW_NONE, FW_FAILED /* or in flight */, FW_VALID, FW_NEW_GRID, FW_BATCH, FW_NEW_COST };
    enum Backward { BW_NOT_REQUESTED, BW_PENDING, BW_COMPLETE, BW_FAILED /* or in flight */ };
    // the last event since the forward half of a split product; TN_NONE until the first one begins, whatever else happens
    enum Tangent { TN_NONE, TN_READY, TN_FAILED /* or in flight */, TN_EVAL, TN_GRID, TN_BATCH, TN_COST, TN_HVP };
    // one state, two wordings: the Hessian-vector calls need the forward sweep, grape_expect speaks of the evaluation -- and
    // counts a backward half that failed behind a good forward half as a failed evaluation
    enum Wording { SWEEP, EVALUATION };

    bool open = false;             // an open-system handle: the names in the sentences, the running-cost refusal
    Forward forward = FW_NONE;
    Backward backward = BW_NOT_REQUESTED;
    // what the last successful backward half was, for the time gradients and the Hessian calls (kept until the next one)
    bool unit = false;             // ... d_bw holds the unit backward states (factor z_k instead of rho_k)
    bool xi_user = false;          // ... the caller's xi (closed: no explicit weight term) or, open, any running cost carried
    bool chi_user = false;         // ... the caller's chi_k(T) (open: still in d_chi)
    Tangent tangent = TN_NONE;
    int nv = 0;                    // directions of the last successful forward half of a split product
    double terms_fw = 0., steps_fw = 0.;   // ... and its statistics, for the info of the backward half

    // ---- events -------------------------------------------------------------------------------------------------------
    // An open handle waits inside the call, so its halves begin as failed and succeed at the end.  A closed forward half
    // counts as present from its enqueue (forward_succeeded there) and is withdrawn by forward_failed wherever the flags of
    // the stream are read: after either half, or at the one wait of grape_eval.
    void forward_begun() { forward = FW_FAILED; backward = BW_NOT_REQUESTED; came(TN_EVAL); }
    void forward_succeeded(bool want_gradient = true) {
        forward = FW_VALID; backward = want_gradient ? BW_PENDING : BW_NOT_REQUESTED; came(TN_EVAL);
    }
    void forward_failed() { forward = FW_FAILED; }   // (the stored states of a failed sweep are nobody's input)
    void no_gradient() { backward = BW_NOT_REQUESTED; }
    void backward_failed() { backward = BW_FAILED; }   // (the forward states stand: grape_open_hvp may still read them)
    void backward_succeeded(bool unit_, bool xi_user_, bool chi_user_) {
        backward = BW_COMPLETE; unit = unit_; xi_user = xi_user_; chi_user = chi_user_;
    }
    // a replay of the captured evaluation: both halves of the built-in functional, with the captured attribute
    void replayed(bool unit_) { forward_succeeded(); backward_succeeded(unit_, false, false); }
    void new_grid() { forward = FW_NEW_GRID; backward = BW_NOT_REQUESTED; came(TN_GRID); }
    void batch_call() { forward = FW_BATCH; came(TN_BATCH); }   // (the per-trajectory terms of a backward half stay readable)
    void new_cost() { forward = FW_NEW_COST; backward = BW_NOT_REQUESTED; came(TN_COST); }
    void tangent_overwritten() { came(TN_HVP); }   // grape_hvp / grape_open_hvp share the tangent storage
    void split_forward_begun() { tangent = TN_FAILED; }
    void split_forward_succeeded(int nv_, double terms, double steps) { tangent = TN_READY; nv = nv_; terms_fw = terms; steps_fw = steps; }

    // ---- queries ------------------------------------------------------------------------------------------------------
    // the clause after "no valid forward state: " (nullptr: the stored forward states are those of one successful forward half
    // on the current grid)
    const char *forward_stale(Wording w = SWEEP) const {
        switch (forward) {
        case FW_VALID: return w == EVALUATION && backward == BW_FAILED ? "the last evaluation failed" : nullptr;
        case FW_NONE: return "no evaluation on this handle yet";
        case FW_NEW_GRID: return "grape_set_tlist came after the last evaluation, the stored states belong to the previous grid";
        case FW_NEW_COST: return "grape_open_set_running_cost came after the last evaluation";
        case FW_BATCH: return "the last call was grape_eval_batch, the stored states are not those of one defined evaluation";
        default: return w == SWEEP ? "the last forward sweep failed" : "the last evaluation failed";
        }
    }
    // what the closed Hessian-vector calls say instead, whatever forward_stale() names
    static constexpr const char *no_forward_on_grid =
        "no valid forward state on this time grid (no evaluation yet, the last one failed, grape_set_tlist came since, "
        "or the last call was grape_eval_batch)";

    // the per-trajectory terms of a backward half are on the device (grape_get_tau_grads of an open handle)
    bool backward_complete() const { return backward == BW_COMPLETE; }

    // the two time gradients: a complete backward half behind the valid forward half
    static constexpr const char *between_halves = "called between grape_forward and the backward half";
    const char *gradient_stale() const {
        if (forward == FW_VALID) switch (backward) {
            case BW_NOT_REQUESTED: return "the last evaluation had no gradient (grape_eval with G == NULL)";
            case BW_PENDING: return between_halves;
            case BW_COMPLETE:
                return open && xi_user ? "the last backward half carried a state running cost (grape_open_set_running_cost or "
                                         "grape_open_backward_xi): the time-gradient kernel does not carry the inhomogeneity"
                                       : nullptr;
            default: break;
        }
        if (!open) return "no complete gradient evaluation on this time grid (none yet, the last one failed, or grape_set_tlist came after it)";
        switch (forward) {
        case FW_NONE: return "no evaluation on this handle yet";
        case FW_NEW_GRID: return "grape_set_tlist came after the last evaluation: the stored states belong to the previous grid";
        case FW_BATCH: return "the last call was grape_eval_batch: the stored states are not those of one defined evaluation";
        case FW_NEW_COST: return "grape_open_set_running_cost came after the last evaluation: its backward half belongs to the previous cost";
        default: return "the last evaluation failed";
        }
    }

    // the backward halves of the split products: the tangent states of a forward half of nv directions, untouched since
    // (empty: go ahead)
    std::string tangent_stale(int nv_) const {
        const std::string fw = open ? "grape_open_hvp_forward" : "grape_hvp_forward";
        switch (tangent) {
        case TN_READY: break;
        case TN_NONE: return "no " + fw + " on this handle yet";
        case TN_EVAL: return "a forward evaluation came since the last " + fw;
        case TN_GRID: return "grape_set_tlist came since the last " + fw;
        case TN_BATCH: return "grape_eval_batch came since the last " + fw;
        case TN_COST: return "grape_open_set_running_cost came since the last " + fw;
        case TN_HVP:
            return (open ? "grape_open_hvp" : "grape_hvp") + (" came since the last " + fw) + " (it shares the tangent storage and overwrites it)";
        default: return "the last " + fw + " failed";
        }
        if (forward_stale()) return "no valid forward state on this time grid";
        if (nv_ != nv) return "nv = " + std::to_string(nv_) + ", but the last " + fw + " took nv = " + std::to_string(nv);
        return std::string();
    }

private:
    void came(Tangent what) { if (tangent != TN_NONE) tangent = what; }
};
