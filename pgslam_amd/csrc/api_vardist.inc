// api_vardist.inc -- part of pgicp_api.cpp (one translation unit): include/pgicp_vardist.h -- arming a matching call with its readings'
// search radii (KDTreeVarDistMatcher), the armed call's look at them, and the cut of the matcher's pairs (k_vardist.inc).

template <typename T>
int arm_reading_radii(pgicp_ctx *c, int P, const T *const *radii, const int *stride, const int *n, int mem)
{
    if (!c) return PGICP_ERR_ARG;
    return arm_rows<T>(c, c->vd, "pgicp_arm_reading_radii", true, launch_vardist_stage<T>, P, radii, stride, n, mem);
}

// Armed radii are consumed by the matching call that finds them, whatever becomes of that call.  A VarDistCall stands at the head
// of every such entry point: it takes the arm, and -- once check() has passed -- the call's iterations cut (c->vd.on) until it returns.
struct VarDistCall {
    pgicp_ctx *c;
    bool armed = false;
    explicit VarDistCall(pgicp_ctx *ctx) : c(ctx)
    {
        if (!c) return;
        armed = c->vd.armed;
        c->vd.armed = false;
        c->vd.on = false;
    }
    ~VarDistCall() { if (c) c->vd.on = false; }
    template <typename T>
    int check(int P, const pgicp_problem *pr)
    {
        if (!armed) return PGICP_OK;
        const int st = rows_check<T>(c, c->vd, "reading radii", "a value is negative or a NaN", P, pr);
        if (st == PGICP_OK) c->vd.on = true;
        return st;
    }
};

// the per-pair arrays everything downstream of the matcher reads in this call: the cut pairs of an armed call, else the matcher's own
template <typename T> int *pair_slots(pgicp_ctx *c) { return c->vd.on ? c->vd.slot_cut.as<int>() : state<T>(c).slot.template as<int>(); }
template <typename T> T *pair_d2(pgicp_ctx *c) { return c->vd.on ? c->vd.d2_cut.as<T>() : state<T>(c).d2.template as<T>(); }

// batch_begin of an armed call: room for the cut pairs (`pairs`: points x knn over the batch)
template <typename T>
int vardist_begin(pgicp_ctx *c, size_t pairs)
{
    c->vd.cut_live = c->vd.on;
    if (!c->vd.on) return PGICP_OK;
    HIPC(c, c->vd.slot_cut.ensure(sizeof(int) * pairs));
    HIPC(c, c->vd.d2_cut.ensure(sizeof(T) * pairs));
    return PGICP_OK;
}

// the cut, behind a matcher pass that resolved every pair of the active problems exactly
template <typename T>
void vardist_cut_enqueue(pgicp_ctx *c, int n_active, int max_pairs)
{
    State<T> &S = state<T>(c);
    launch_vardist_cut<T>(c->stream, c->probs.as<ProblemDev>(), c->active.as<int>(), n_active, max_pairs, S.slot.template as<int>(),
                          S.d2.template as<T>(), c->order.as<int>(), c->vd.vals.template as<T>(), c->vd.off_dev.as<long long>(),
                          c->vd.slot_cut.as<int>(), c->vd.d2_cut.as<T>());
}
