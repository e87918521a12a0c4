// Stand-alone check of csrc/grape_evalstate.h under -fsanitize=address,undefined (tests/test_evalstate_host.py builds and runs it).
// The header is plain C++: no HIP call to define, nothing to link.
//
// Part 1 walks every sequence of at most six events over the events a closed and an open handle can see and holds the record,
// after every prefix, against a model that keeps nothing but "what happened last".  Part 2 is the table of every refusal a
// caller can read, consumer by reachable state, as the library worded them before the record existed: the sentences of
// grape_hip.hip are composed from the header's clauses, so a changed word in either fails here, without a GPU.
#include "grape_evalstate.h"

#include <array>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

namespace {

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

enum Event { FWD_BEGUN, FWD_OK, FWD_OK_NO_GRADIENT, FWD_FAILED, BWD_OK, BWD_OK_XI, BWD_FAILED, NO_GRADIENT, REPLAY, GRID, BATCH, COST,
             HVP, SPLIT_BEGUN, SPLIT_OK };
const char *const kEventName[] = {"forward_begun", "forward_succeeded", "forward_succeeded(false)", "forward_failed", "backward_succeeded",
                                  "backward_succeeded(xi)", "backward_failed", "no_gradient", "replayed", "new_grid", "batch_call", "new_cost",
                                  "tangent_overwritten", "split_forward_begun", "split_forward_succeeded"};
constexpr int NV = 2;   // directions of every split forward half of the walk

void apply(StoredEval &r, Event e) {
    switch (e) {
    case FWD_BEGUN: r.forward_begun(); break;
    case FWD_OK: r.forward_succeeded(); break;
    case FWD_OK_NO_GRADIENT: r.forward_succeeded(false); break;
    case FWD_FAILED: r.forward_failed(); break;
    case BWD_OK: r.backward_succeeded(false, false, false); break;
    case BWD_OK_XI: r.backward_succeeded(false, true, false); break;
    case BWD_FAILED: r.backward_failed(); break;
    case NO_GRADIENT: r.no_gradient(); break;
    case REPLAY: r.replayed(true); break;
    case GRID: r.new_grid(); break;
    case BATCH: r.batch_call(); break;
    case COST: r.new_cost(); break;
    case HVP: r.tangent_overwritten(); break;
    case SPLIT_BEGUN: r.split_forward_begun(); break;
    case SPLIT_OK: r.split_forward_succeeded(NV, 10., 1.); break;
    }
}

// what the model remembers: the last event of each kind, nothing derived from the record
struct Model {
    bool fwd_good = false;        // the last forward event was a success and no grid, batch or cost event came after it
    bool bwd_complete = false;    // a backward half has succeeded since, with nothing that withdraws it after
    bool bwd_xi = false;          // ... and carried a running cost
    bool split_seen = false;      // a split forward half has begun or succeeded on this record
    Event tangent_last = SPLIT_BEGUN;   // the last event that touched the tangent storage since (meaningful once split_seen)
    void apply(Event e) {
        switch (e) {
        case FWD_BEGUN: fwd_good = false; bwd_complete = false; break;
        case FWD_FAILED: fwd_good = false; break;   // (the terms a backward half left are still its own)
        case FWD_OK: case FWD_OK_NO_GRADIENT: fwd_good = true; bwd_complete = false; break;
        case BWD_OK: case BWD_OK_XI: bwd_complete = true; bwd_xi = e == BWD_OK_XI; break;
        case BWD_FAILED: case NO_GRADIENT: bwd_complete = false; break;
        case REPLAY: fwd_good = true; bwd_complete = true; bwd_xi = false; break;
        case GRID: case COST: fwd_good = false; bwd_complete = false; break;
        case BATCH: fwd_good = false; break;
        default: break;
        }
        if (e == SPLIT_BEGUN || e == SPLIT_OK) { split_seen = true; tangent_last = e; }
        else if (split_seen && (e == FWD_BEGUN || e == FWD_OK || e == FWD_OK_NO_GRADIENT || e == REPLAY || e == GRID || e == BATCH || e == COST || e == HVP))
            tangent_last = e;
    }
};

std::string came_since(bool open, Event last) {
    const std::string fw = open ? "grape_open_hvp_forward" : "grape_hvp_forward";
    switch (last) {
    case SPLIT_BEGUN: return "the last " + fw + " failed";
    case GRID: return "grape_set_tlist came since the last " + fw;
    case BATCH: return "grape_eval_batch came since the last " + fw;
    case COST: return "grape_open_set_running_cost came since the last " + fw;
    case HVP: return std::string(open ? "grape_open_hvp" : "grape_hvp") + " came since the last " + fw + " (it shares the tangent storage and overwrites it)";
    default: return "a forward evaluation came since the last " + fw;
    }
}

long g_nodes = 0;
std::vector<Event> g_path;

void fail_path(const char *what) {
    std::printf("FAILED invariant: %s, after", what);
    for (Event e : g_path) std::printf(" %s", kEventName[e]);
    std::printf("\n");
    std::exit(1);
}
#define INVARIANT(cond, what) do { if (!(cond)) fail_path(what); } while (0)

void check(const StoredEval &r, const Model &m) {
    ++g_nodes;
    const bool open = r.open;
    // no consumer accepts unless the last forward event was a success with no staling event after it -- and the two queries
    // for the forward states accept whenever it was (the evaluation wording: unless a backward half failed behind it)
    INVARIANT((r.forward_stale() == nullptr) == m.fwd_good, "forward_stale() accepts iff the forward states are good");
    INVARIANT(r.forward_stale(StoredEval::EVALUATION) != nullptr || m.fwd_good, "forward_stale(EVALUATION) accepts only good forward states");
    INVARIANT(r.forward_stale(StoredEval::EVALUATION) == nullptr || r.forward_stale() != nullptr || r.backward == StoredEval::BW_FAILED,
              "the two wordings differ only behind a failed backward half");
    // the time gradient accepts only with a complete backward half after that forward half
    const bool tg = r.gradient_stale() == nullptr;
    INVARIANT(tg == (m.fwd_good && m.bwd_complete && !(open && m.bwd_xi)), "gradient_stale() accepts iff a backward half completed after the forward half");
    INVARIANT(!r.backward_complete() || m.bwd_complete, "backward_complete() only after a backward half that succeeded");
    // a backward half of a split product accepts only if nothing came since its forward half and nv matches; the reason is
    // the last intervening event; before the first split forward half it is "no ... yet", whatever else happened
    const std::string same = r.tangent_stale(NV), other = r.tangent_stale(NV + 1);
    const std::string fw = open ? "grape_open_hvp_forward" : "grape_hvp_forward";
    if (!m.split_seen) {
        INVARIANT(same == "no " + fw + " on this handle yet" && other == same, "before the first split forward half: no ... yet");
    } else if (m.tangent_last != SPLIT_OK) {
        INVARIANT(same == came_since(open, m.tangent_last) && other == same, "tangent_stale() names the last intervening event");
    } else if (!m.fwd_good) {
        INVARIANT(same == "no valid forward state on this time grid" && other == same, "tangent_stale() refuses stale forward states");
    } else {
        INVARIANT(same.empty(), "tangent_stale() accepts an untouched forward half of the same nv");
        INVARIANT(other == "nv = 3, but the last " + fw + " took nv = 2", "tangent_stale() refuses another nv");
    }
}

// Every sequence, not every sequence anew: what follows a prefix depends on nothing but the record, the model and the events
// left, so a prefix that ends where an earlier one of the same length ended has had all its continuations walked already.
std::set<std::array<int, 15>> g_seen;

void walk(const StoredEval &r, const Model &m, const std::vector<Event> &alphabet, int depth) {
    const std::array<int, 15> key = {r.open, r.forward, r.backward, r.unit, r.xi_user, r.chi_user, r.tangent, r.nv, (int)r.terms_fw,
                                     (int)r.steps_fw, m.fwd_good, m.bwd_complete, m.bwd_xi, m.split_seen * 100 + m.tangent_last, depth};
    if (!g_seen.insert(key).second) return;
    check(r, m);
    if (depth == 0) return;
    for (Event e : alphabet) {
        StoredEval r2 = r;
        Model m2 = m;
        apply(r2, e);
        m2.apply(e);
        g_path.push_back(e);
        walk(r2, m2, alphabet, depth - 1);
        g_path.pop_back();
    }
}

// ---- part 2: the sentences -----------------------------------------------------------------------------------------------

StoredEval after(bool open, const std::vector<Event> &events) {
    StoredEval r;
    r.open = open;
    for (Event e : events) apply(r, e);
    return r;
}

void expect_eq(const std::string &got, const char *want) {
    if (got != want) { std::printf("FAILED sentence:\n  got  \"%s\"\n  want \"%s\"\n", got.c_str(), want); std::exit(1); }
}

// as grape_hip.hip composes them
std::string stale_forward(const char *call, const StoredEval &r, StoredEval::Wording w) {
    const char *why = r.forward_stale(w);
    return why ? std::string(call) + ": no valid forward state: " + why : std::string();
}
std::string closed_coarse(const char *call, const StoredEval &r) {
    return r.forward_stale() ? std::string(call) + ": " + StoredEval::no_forward_on_grid : std::string();
}
std::string time_gradient(const StoredEval &r) {
    const char *why = r.gradient_stale();
    if (!why) return std::string();
    if (r.open) return std::string("grape_open_time_gradient: ") + why;
    return std::string("grape_get_time_gradient") + (why == StoredEval::between_halves ? " " : ": ") + why;
}
std::string split_backward(const char *call, const StoredEval &r, int nv) {
    const std::string why = r.tangent_stale(nv);
    return why.empty() ? why : std::string(call) + ": " + why;
}

void table() {
    const bool O = true, C = false;
    // grape_open_time_gradient, one row per TG_* value of the parent
    expect_eq(time_gradient(after(O, {})), "grape_open_time_gradient: no evaluation on this handle yet");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, NO_GRADIENT})), "grape_open_time_gradient: the last evaluation had no gradient (grape_eval with G == NULL)");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK})), "grape_open_time_gradient: called between grape_forward and the backward half");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED, BWD_OK})), "");
    expect_eq(time_gradient(after(O, {FWD_BEGUN})), "grape_open_time_gradient: the last evaluation failed");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED})), "grape_open_time_gradient: the last evaluation failed");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED, BWD_OK, GRID})),
              "grape_open_time_gradient: grape_set_tlist came after the last evaluation: the stored states belong to the previous grid");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED, BWD_OK, BATCH})),
              "grape_open_time_gradient: the last call was grape_eval_batch: the stored states are not those of one defined evaluation");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED, BWD_OK, COST})),
              "grape_open_time_gradient: grape_open_set_running_cost came after the last evaluation: its backward half belongs to the previous cost");
    expect_eq(time_gradient(after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED, BWD_OK_XI})),
              "grape_open_time_gradient: the last backward half carried a state running cost (grape_open_set_running_cost or "
              "grape_open_backward_xi): the time-gradient kernel does not carry the inhomogeneity");

    // the three sentences of grape_get_time_gradient; a caller's xi is no refusal on a closed handle
    const char *tg0 = "grape_get_time_gradient: no complete gradient evaluation on this time grid (none yet, the last one failed, or "
                      "grape_set_tlist came after it)";
    expect_eq(time_gradient(after(C, {})), tg0);
    expect_eq(time_gradient(after(C, {FWD_OK, BWD_OK, FWD_FAILED})), tg0);
    expect_eq(time_gradient(after(C, {FWD_OK, BWD_OK, GRID})), tg0);
    expect_eq(time_gradient(after(C, {FWD_OK, BWD_OK, BATCH})), tg0);
    expect_eq(time_gradient(after(C, {FWD_OK_NO_GRADIENT})), "grape_get_time_gradient: the last evaluation had no gradient (grape_eval with G == NULL)");
    expect_eq(time_gradient(after(C, {FWD_OK})), "grape_get_time_gradient called between grape_forward and the backward half");
    expect_eq(time_gradient(after(C, {FWD_OK, BWD_OK})), "");
    expect_eq(time_gradient(after(C, {FWD_OK, BWD_OK_XI})), "");
    expect_eq(time_gradient(after(C, {FWD_OK_NO_GRADIENT, REPLAY})), "");

    // the five open "no valid forward state: ..." sentences, in the wording of the Hessian-vector calls (grape_open_hvp,
    // grape_open_hvp_forward, grape_open_hessian) and in that of grape_expect
    struct Row { std::vector<Event> events; const char *sweep, *evaluation; };
    const Row rows[] = {
        {{}, "no valid forward state: no evaluation on this handle yet", "no valid forward state: no evaluation on this handle yet"},
        {{FWD_BEGUN, FWD_OK, GRID},
         "no valid forward state: grape_set_tlist came after the last evaluation, the stored states belong to the previous grid",
         "no valid forward state: grape_set_tlist came after the last evaluation, the stored states belong to the previous grid"},
        {{FWD_BEGUN, FWD_OK, COST}, "no valid forward state: grape_open_set_running_cost came after the last evaluation",
         "no valid forward state: grape_open_set_running_cost came after the last evaluation"},
        {{FWD_BEGUN, FWD_OK, BATCH},
         "no valid forward state: the last call was grape_eval_batch, the stored states are not those of one defined evaluation",
         "no valid forward state: the last call was grape_eval_batch, the stored states are not those of one defined evaluation"},
        {{FWD_BEGUN}, "no valid forward state: the last forward sweep failed", "no valid forward state: the last evaluation failed"},
    };
    for (const Row &row : rows) {
        const StoredEval r = after(O, row.events);
        for (const char *call : {"grape_open_hvp", "grape_open_hvp_forward", "grape_open_hessian"})
            expect_eq(stale_forward(call, r, StoredEval::SWEEP), (std::string(call) + ": " + row.sweep).c_str());
        expect_eq(stale_forward("grape_expect", r, StoredEval::EVALUATION), (std::string("grape_expect: ") + row.evaluation).c_str());
    }
    // a backward half that failed behind a good forward half: the Hessian-vector calls go ahead, grape_expect refuses
    expect_eq(stale_forward("grape_open_hvp", after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED}), StoredEval::SWEEP), "");
    expect_eq(stale_forward("grape_expect", after(O, {FWD_BEGUN, FWD_OK, BWD_FAILED}), StoredEval::EVALUATION),
              "grape_expect: no valid forward state: the last evaluation failed");
    expect_eq(stale_forward("grape_expect", after(O, {FWD_BEGUN, FWD_OK, NO_GRADIENT}), StoredEval::EVALUATION), "");
    // grape_expect on a closed handle (a composite asks its shards the same)
    expect_eq(stale_forward("grape_expect", after(C, {}), StoredEval::EVALUATION), "grape_expect: no valid forward state: no evaluation on this handle yet");
    expect_eq(stale_forward("grape_expect", after(C, {FWD_OK, FWD_FAILED}), StoredEval::EVALUATION),
              "grape_expect: no valid forward state: the last evaluation failed");
    expect_eq(stale_forward("grape_expect", after(C, {FWD_OK, GRID}), StoredEval::EVALUATION),
              "grape_expect: no valid forward state: grape_set_tlist came after the last evaluation, the stored states belong to the previous grid");
    expect_eq(stale_forward("grape_expect", after(C, {FWD_OK, BATCH}), StoredEval::EVALUATION),
              "grape_expect: no valid forward state: the last call was grape_eval_batch, the stored states are not those of one defined evaluation");
    expect_eq(stale_forward("grape_expect", after(C, {FWD_OK_NO_GRADIENT}), StoredEval::EVALUATION), "");

    // grape_hvp, grape_hessian, grape_hvp_forward: one coarse sentence whatever the reason
    for (const char *call : {"grape_hvp", "grape_hessian", "grape_hvp_forward"}) {
        const std::string want = std::string(call) + ": no valid forward state on this time grid (no evaluation yet, the last one failed, "
                                 "grape_set_tlist came since, or the last call was grape_eval_batch)";
        expect_eq(closed_coarse(call, after(C, {})), want.c_str());
        expect_eq(closed_coarse(call, after(C, {FWD_OK, FWD_FAILED})), want.c_str());
        expect_eq(closed_coarse(call, after(C, {FWD_OK, GRID})), want.c_str());
        expect_eq(closed_coarse(call, after(C, {FWD_OK, BWD_OK, BATCH})), want.c_str());
        expect_eq(closed_coarse(call, after(C, {FWD_OK_NO_GRADIENT})), "");
        expect_eq(closed_coarse(call, after(C, {REPLAY})), "");
    }

    // the backward halves of the split products: seven closed sentences ...
    const char *cb = "grape_hvp_backward";
    expect_eq(split_backward(cb, after(C, {FWD_OK, BATCH, GRID, HVP}), NV), "grape_hvp_backward: no grape_hvp_forward on this handle yet");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, FWD_OK}), NV),
              "grape_hvp_backward: a forward evaluation came since the last grape_hvp_forward");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, REPLAY}), NV),
              "grape_hvp_backward: a forward evaluation came since the last grape_hvp_forward");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, GRID}), NV), "grape_hvp_backward: grape_set_tlist came since the last grape_hvp_forward");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, GRID, BATCH}), NV),
              "grape_hvp_backward: grape_eval_batch came since the last grape_hvp_forward");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, HVP}), NV),
              "grape_hvp_backward: grape_hvp came since the last grape_hvp_forward (it shares the tangent storage and overwrites it)");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN}), NV), "grape_hvp_backward: the last grape_hvp_forward failed");
    expect_eq(split_backward("grape_hvp_backward_chi", after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, FWD_FAILED}), NV),
              "grape_hvp_backward_chi: no valid forward state on this time grid");
    // ... eight open ones ...
    const char *ob = "grape_open_hvp_backward";
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, COST, HVP}), NV), "grape_open_hvp_backward: no grape_open_hvp_forward on this handle yet");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, FWD_BEGUN}), NV),
              "grape_open_hvp_backward: a forward evaluation came since the last grape_open_hvp_forward");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, GRID}), NV),
              "grape_open_hvp_backward: grape_set_tlist came since the last grape_open_hvp_forward");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, BATCH}), NV),
              "grape_open_hvp_backward: grape_eval_batch came since the last grape_open_hvp_forward");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, BATCH, COST}), NV),
              "grape_open_hvp_backward: grape_open_set_running_cost came since the last grape_open_hvp_forward");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, HVP}), NV),
              "grape_open_hvp_backward: grape_open_hvp came since the last grape_open_hvp_forward (it shares the tangent storage and overwrites it)");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN}), NV), "grape_open_hvp_backward: the last grape_open_hvp_forward failed");
    expect_eq(split_backward("grape_open_hvp_backward_chi", after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, FWD_FAILED}), NV),
              "grape_open_hvp_backward_chi: no valid forward state on this time grid");
    // ... the nv mismatch, and the go-ahead (a failed backward half of the evaluation does not touch the tangent storage)
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK}), 5), "grape_hvp_backward: nv = 5, but the last grape_hvp_forward took nv = 2");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK}), 1),
              "grape_open_hvp_backward: nv = 1, but the last grape_open_hvp_forward took nv = 2");
    expect_eq(split_backward(cb, after(C, {FWD_OK, SPLIT_BEGUN, SPLIT_OK, BWD_OK}), NV), "");
    expect_eq(split_backward(ob, after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN, SPLIT_OK, BWD_FAILED}), NV), "");

    // what the backward half left: the attributes the time gradients and the Hessian calls read stay until the next one
    StoredEval r = after(C, {FWD_OK});
    r.backward_succeeded(true, true, false);
    CHECK(r.unit && r.xi_user && !r.chi_user);
    r.forward_succeeded();
    CHECK(r.unit && r.xi_user);                 // (grape_hessian refuses on xi_user before it asks for the forward states)
    r.replayed(false);
    CHECK(!r.unit && !r.xi_user && !r.chi_user && r.gradient_stale() == nullptr);
    r = after(O, {FWD_BEGUN, FWD_OK});
    r.backward_succeeded(false, false, true);
    CHECK(r.chi_user && r.backward_complete());
    r.batch_call();
    CHECK(r.backward_complete());               // (grape_get_tau_grads of an open handle after a batch call)
    r.new_cost();
    CHECK(!r.backward_complete());
    r = after(O, {FWD_BEGUN, FWD_OK, SPLIT_BEGUN});
    r.split_forward_succeeded(3, 42., 7.);
    CHECK(r.nv == 3 && r.terms_fw == 42. && r.steps_fw == 7.);
}

}  // namespace

int main() {
    const std::vector<Event> closed = {FWD_OK, FWD_OK_NO_GRADIENT, FWD_FAILED, BWD_OK, BWD_OK_XI, REPLAY, GRID, BATCH, HVP, SPLIT_BEGUN, SPLIT_OK};
    const std::vector<Event> open = {FWD_BEGUN, FWD_OK, FWD_FAILED, BWD_OK, BWD_OK_XI, BWD_FAILED, NO_GRADIENT, GRID, BATCH, COST, HVP, SPLIT_BEGUN, SPLIT_OK};
    StoredEval c, o;
    o.open = true;
    walk(c, Model(), closed, 6);
    const long closed_nodes = g_nodes;
    walk(o, Model(), open, 6);
    table();
    std::printf("evalstate-driver OK (every sequence of at most 6 of %zu closed and %zu open events: %ld and %ld distinct situations)\n",
                closed.size(), open.size(), closed_nodes, g_nodes - closed_nodes);
    return 0;
}
