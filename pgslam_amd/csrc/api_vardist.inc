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

// batch_begin of an armed call: room for the cut pairs (`pairs`: points x knn over the batch).  The call's IterBufs (api_icp.inc) then
// names them as the pairs everything behind the matcher reads, and cut_pairs fills them.
template <typename T>
int vardist_begin(pgicp_ctx *c, size_t pairs)
{
    c->vd.cut_live = c->vd.on;
    if (!c->vd.on) return PGICP_OK;
    HIPC(c, c->vd.slot_cut.ensure(sizeof(int) * pairs));
    HIPC(c, c->vd.d2_cut.ensure(sizeof(T) * pairs));
    return PGICP_OK;
}
