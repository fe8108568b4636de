// tracers.hip -- tracer sets (include/xpic_tracers.h): batches of test particles that the context owns and
// that stay on the device between calls, so that they can follow E and B through a run (xpic_step carries the attached
// sets, api.hip).  There is no kernel here.  A set is advanced by the open traces' own launches (fo_launch_open,
// dk_launch_open: trace_call.h) through the launch loop the open traces run (trace_launches, LiveList: batch.h) and
// compacted by trace_open.hip; what this file adds is the ownership of the arrays batch_trace stages for one call, the
// bookkeeping that turns a set's life into one long call, and the sample buffer of fixed capacity.  The set itself is
// tracer_set.h's, which tracer_moments.hip shares: the maps of a set take their deposits between the launches of advance.
//
// One long call: the kernels count steps from `first` (steps of the call before the launch), write sample row
// step / sample_every - 1 while it is < nsamp, and set exit_step = R.step0 + first + the steps completed.  A set that has
// made `done` steps, `base` sample rows of which have left the buffer (drained or dropped), launches with
// first = done - base * sample_every and R.step0 = step0 + base * sample_every: the sum, and so exit_step, is the
// open trace's, a step is sampled iff `done` reaches a multiple of sample_every, and the rows count from the buffer's row 0.
#include <algorithm>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "batch.h"
#include "common.h"
#include "trace_call.h"
#include "trace_open.h"
#include "tracer_set.h"

namespace xpic {

int tracers_find(xpic_ctx* ctx, const std::string& who, int id, TracerSet** out)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  if (ctx->tracers)
    for (auto& t : ctx->tracers->sets)
      if (t->id == id) { *out = t.get(); return 0; }
  XPIC_CHECK(false, who + ": set " + std::to_string(id) + " does not exist (never created, or destroyed)");
  return 0;
}

namespace {

int find_set(xpic_ctx* ctx, const std::string& who, int id, TracerSet** out) { return tracers_find(ctx, who, id, out); }

bool wants_gradient(const TracerSet& T)
{
  return T.kind == XPIC_TRACERS_DRIFT_KINETIC && T.gradB == XPIC_GRADB_AUTO && T.n > 0;
}

// XPIC_GRADB_AUTO: grad |B| of the context's B as it stands, into the set layer's own vector
int auto_gradient(xpic_ctx* ctx)
{
  TracerSets& S = *ctx->tracers;
  if (!S.gradB) XPIC_HIP(hipMalloc(&S.gradB, sizeof(double) * ctx->nvec));
  return grad_abs_field(ctx, ctx->field[XPIC_B], S.gradB);
}

// `steps` >= 0 steps of one set on the context's fields as they stand.  have_gradient: the caller has run auto_gradient on
// this B already (a ride computes it once for all its sets)
int advance_plain(xpic_ctx* ctx, TracerSet& T, int64_t steps, bool have_gradient)
{
  if (T.n > 0 && steps > 0) {
    const bool dk = T.kind == XPIC_TRACERS_DRIFT_KINETIC;
    const double* gB = nullptr;
    if (wants_gradient(T)) {
      if (!have_gradient) XPIC_CALL(auto_gradient(ctx));
      gB = ctx->tracers->gradB;
    } else if (dk && T.gradB >= 0) {
      gB = ctx->field[T.gradB];
    }
    TraceDev d{};
    d.s = T.s.p; d.samples = T.sm.p; d.nsamp = (long)(T.sm.p ? T.cap : 0);
    d.it_sum = (long long*)T.tot.p; d.it_max = T.mx.p; d.exit_step = (long long*)T.ex.p;
    d.alive = (unsigned long long*)T.al.p; d.removed = (unsigned long long*)T.rm.p;
    const int64_t shift = T.base * T.every; // steps that lie before the buffer's row 0
    OpenRegion R = T.R;
    R.step0 += shift;
    const long n = (long)T.n, every = (long)std::max<int64_t>(T.every, 1);
    if (dk)
      XPIC_CALL(trace_launches(ctx, "tracers_dk", "tracers_dk_compact", XPIC_DK_LAUNCH_STEPS, T.done - shift, steps, T.policy,
        T.tracked, d, T.L, [&](const TraceDev& l) { dk_launch_open(ctx, T.dk, gB, R, n, every, l); }));
    else
      XPIC_CALL(trace_launches(ctx, "tracers_fo", "tracers_fo_compact", XPIC_FO_LAUNCH_STEPS, T.done - shift, steps, T.policy,
        T.tracked, d, T.L, [&](const TraceDev& l) { fo_launch_open(ctx, T.fo, R, n, every, l); }));
  }
  T.done += steps;
  return 0;
}

// advance_plain for a set without maps.  With maps the steps are split where one of them is due (the set's step count
// reaches a multiple of its `every`) and the deposit runs between the trace launches: by composition ((2) in
// include/xpic_tracers.h) the set's own bits are those of the unsplit advance.  B does not change during the call, so
// the pieces share one gradient.
int advance(xpic_ctx* ctx, TracerSet& T, int64_t steps, bool have_gradient = false)
{
  if (T.maps.empty()) return advance_plain(ctx, T, steps, have_gradient);
  while (steps > 0) {
    int64_t piece = steps;
    for (auto& m : T.maps) piece = std::min(piece, m->every - T.done % m->every);
    XPIC_CALL(advance_plain(ctx, T, piece, have_gradient));
    have_gradient = have_gradient || wants_gradient(T);
    XPIC_CALL(tracer_maps_deposit(ctx, T));
    steps -= piece;
  }
  return 0;
}

}  // namespace

int tracers_ride(xpic_ctx* c)
{
  bool have_gradient = false; // B does not change during a ride: its attached sets share one gradient
  for (auto& t : c->tracers->sets) {
    if (!t->attached) continue;
    if (wants_gradient(*t) && !have_gradient) {
      XPIC_CALL(auto_gradient(c));
      have_gradient = true;
    }
    XPIC_CALL(advance(c, *t, 1, have_gradient));
  }
  return 0;
}

void tracers_free(xpic_ctx* c)
{
  if (!c->tracers) return;
  (void)hipFree(c->tracers->gradB);
  delete c->tracers;
  c->tracers = nullptr;
}

}  // namespace xpic

using namespace xpic;

extern "C" {

int xpic_grad_abs_field(xpic_ctx* ctx, int src_field, int dst_field)
{
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    "grad_abs_field: a context of several z-slabs (or a self_ring one) is not supported: the kernel wraps z");
  for (int f : {src_field, dst_field})
    XPIC_CHECK(f >= 0 && f < XPIC_NFIELDS && ctx->field[f], "grad_abs_field: unknown or unallocated field id");
  XPIC_CHECK(src_field != dst_field, "grad_abs_field: src_field and dst_field are the same vector");
  return grad_abs_field(ctx, ctx->field[src_field], ctx->field[dst_field]);
}

int xpic_tracers_create(xpic_ctx* ctx, int kind, int64_t n, const void* params, const double* state_6,
  const xpic_trace_region* region, int gradB_field, int64_t sample_every, int64_t sample_capacity, int* set)
{
  const std::string who = "tracers_create";
  XPIC_CHECK(ctx != nullptr, "null context");
  XPIC_CHECK(ctx->geom.nranks == 1 && ctx->g.G == 0,
    who + ": a context of several z-slabs (or a self_ring one) is not supported: the gathers wrap z in the kernel");
  XPIC_CHECK(kind == XPIC_TRACERS_FULL_ORBIT || kind == XPIC_TRACERS_DRIFT_KINETIC, who + ": unknown kind");
  XPIC_CHECK(n >= 0 && n <= ((int64_t)1 << 36), who + ": n is negative or larger than 2^36");
  XPIC_CHECK(set, who + ": set is null");
  XPIC_CHECK(state_6 || n == 0, who + ": state_6 is null");
  XPIC_CHECK(sample_every >= 0 && sample_capacity >= 0, who + ": sample_every or sample_capacity is negative");
  XPIC_CHECK(ctx->field[XPIC_E] && ctx->field[XPIC_B], who + ": the context has no E or B");
  auto T = std::make_unique<TracerSet>();
  T->kind = kind;
  T->n = n;
  if (kind == XPIC_TRACERS_FULL_ORBIT) {
    XPIC_CALL(fo_check_params(who, (const xpic_fo_params*)params));
    T->fo = *(const xpic_fo_params*)params;
  } else {
    XPIC_CALL(dk_check_params(who, (const xpic_dk_params*)params, 0));
    T->dk = *(const xpic_dk_params*)params;
    XPIC_CHECK(gradB_field == XPIC_GRADB_AUTO || gradB_field == -1 ||
        (gradB_field >= 0 && gradB_field < XPIC_NFIELDS && ctx->field[gradB_field]),
      who + ": gradB_field is neither XPIC_GRADB_AUTO, -1 nor an allocated field id");
    T->gradB = gradB_field;
  }
  if (region) {
    XPIC_CALL(trace_region(who, region, false, true, &T->R));
    T->policy = region->compact;
    T->tracked = true;
  } else {
    const double inf = std::numeric_limits<double>::infinity();
    T->R = OpenRegion{XPIC_GEOM_BOX, {-inf, -inf, -inf, inf, inf, inf, 0.0}, 0};
  }
  T->every = sample_every;
  T->cap = sample_every > 0 ? sample_capacity : 0;
  int64_t rows;
  XPIC_CHECK(trace_sample_bytes(n, T->cap, 1, true, &rows) >= 0,
    who + ": the sample buffer (48 n sample_capacity bytes) is too large");
  if (!ctx->tracers) ctx->tracers = new TracerSets;
  TracerSets& S = *ctx->tracers;
  XPIC_CHECK((int)S.sets.size() < XPIC_TRACERS_MAX_SETS,
    who + ": the context already has " + std::to_string(XPIC_TRACERS_MAX_SETS) + " sets");
  T->L.listed = T->L.live = n;
  if (n > 0) {
    std::vector<double> h;
    to_soa(state_6, n, h);
    const std::vector<int64_t> alive(n, -1);
    XPIC_CALL(T->s.alloc(6 * n)); XPIC_CALL(T->ex.alloc(n)); XPIC_CALL(T->rm.alloc(1));
    XPIC_CALL(zero(T->rm, 1, ctx->stream));
    if (T->counters()) {
      XPIC_CALL(T->tot.alloc(n)); XPIC_CALL(T->mx.alloc(n));
      XPIC_CALL(zero(T->tot, n, ctx->stream)); XPIC_CALL(zero(T->mx, n, ctx->stream));
    }
    if (T->cap > 0) {
      XPIC_CALL(T->sm.alloc((size_t)6 * n * T->cap)); XPIC_CALL(T->al.alloc(T->cap));
      XPIC_CALL(zero(T->al, T->cap, ctx->stream));
    }
    XPIC_CALL(upload(T->s, h.data(), 6 * n, ctx->stream));
    XPIC_CALL(upload(T->ex, alive.data(), n, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream)); // the staging vectors end here
  }
  *set = T->id = S.next_id++;
  S.sets.push_back(std::move(T));
  return 0;
}

int xpic_tracers_advance(xpic_ctx* ctx, int set, int64_t steps)
{
  TracerSet* T = nullptr;
  XPIC_CALL(find_set(ctx, "tracers_advance", set, &T));
  XPIC_CHECK(steps >= 0, "tracers_advance: steps is negative");
  return advance(ctx, *T, steps);
}

int xpic_tracers_attach(xpic_ctx* ctx, int set, int on)
{
  TracerSet* T = nullptr;
  XPIC_CALL(find_set(ctx, "tracers_attach", set, &T));
  T->attached = on != 0;
  return 0;
}

int xpic_tracers_get(xpic_ctx* ctx, int set, double* state_6, int64_t* exit_step, int64_t* iterations_sum,
  int* iterations_max, int64_t info5[5])
{
  TracerSet* T = nullptr;
  XPIC_CALL(find_set(ctx, "tracers_get", set, &T));
  const int64_t n = T->n;
  std::vector<double> h(state_6 ? 6 * n : 0);
  int64_t removed = 0;
  if (n > 0) {
    if (state_6) XPIC_CALL(download(h.data(), T->s, 6 * n, ctx->stream));
    if (exit_step) XPIC_CALL(download(exit_step, T->ex, n, ctx->stream));
    if (T->counters()) {
      if (iterations_sum) XPIC_CALL(download(iterations_sum, T->tot, n, ctx->stream));
      if (iterations_max) XPIC_CALL(download(iterations_max, T->mx, n, ctx->stream));
    }
    XPIC_CALL(download(&removed, T->rm, 1, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    if (state_6) to_aos(h.data(), n, state_6);
    if (!T->counters()) { // a Chin id has no iterations
      if (iterations_sum) std::fill(iterations_sum, iterations_sum + n, (int64_t)0);
      if (iterations_max) std::fill(iterations_max, iterations_max + n, 0);
    }
  }
  if (info5) {
    info5[0] = T->done; info5[1] = removed; info5[2] = n - removed; info5[3] = T->held(); info5[4] = T->lost();
  }
  return 0;
}

int xpic_tracers_samples(xpic_ctx* ctx, int set, double* samples, int64_t* alive, int64_t* count)
{
  TracerSet* T = nullptr;
  XPIC_CALL(find_set(ctx, "tracers_samples", set, &T));
  XPIC_CHECK(count, "tracers_samples: count is null");
  const int64_t n = T->n, rows = T->held();
  const size_t row = (size_t)6 * n;
  if (n > 0 && rows > 0) {
    std::vector<double> hs(samples ? row * rows : 0), h(samples ? row : 0), state(samples ? row : 0);
    std::vector<int64_t> ex(samples ? n : 0);
    if (samples) {
      XPIC_CALL(download(hs.data(), T->sm, row * rows, ctx->stream));
      XPIC_CALL(download(h.data(), T->s, row, ctx->stream));
      XPIC_CALL(download(ex.data(), T->ex, n, ctx->stream));
    }
    if (alive) XPIC_CALL(download(alive, T->al, rows, ctx->stream));
    XPIC_CALL(zero(T->al, T->cap, ctx->stream));
    XPIC_HIP(hipStreamSynchronize(ctx->stream));
    if (samples) { // the rows behind a removed particle's last step, as batch_trace fills them
      const std::vector<int64_t> entered(n, -1);
      to_aos(h.data(), n, state.data());
      for (int64_t k = 0; k < rows; ++k) to_aos(hs.data() + row * k, n, samples + row * k);
      fill_frozen_samples(n, rows, T->every, T->R.step0 + T->base * T->every, entered.data(), ex.data(), state.data(), samples);
    }
  } else if (alive) {
    std::fill(alive, alive + rows, (int64_t)0);
  }
  *count = rows;
  T->dropped = T->lost();
  T->base = T->due();
  return 0;
}

int xpic_tracers_destroy(xpic_ctx* ctx, int set)
{
  TracerSet* T = nullptr;
  XPIC_CALL(find_set(ctx, "tracers_destroy", set, &T));
  XPIC_HIP(hipStreamSynchronize(ctx->stream));
  auto& sets = ctx->tracers->sets;
  sets.erase(std::find_if(sets.begin(), sets.end(), [&](const std::unique_ptr<TracerSet>& t) { return t.get() == T; }));
  return 0;
}

}  // extern "C"
