// engine_step.hip -- set_action, the step drivers (one launch | single-sync pipeline | host-checked), get_reward, clear_dead of the host engine
// (GridWorld.cc:403-704)
#include "engine_impl.h"

namespace magent_amd {

// ------------------------------------------------------------------------------------------------ set_action
void Env::set_action_device(int g, const int *d_act) {
    if (g < 0 || g >= (int)groups.size()) fatal("invalid group handle in set_action : %d", g);
    use_device();
    HostGroup &G = groups[g];
    // a group is given actions again before the step: the reference appends (GridWorld.cc:403-454) -- or goals are given actions, which may
    // move them (Map::do_move treats a goal that has taken nobody in like any mover; the parallel move resolution rests on goals that
    // stand still): either way the step runs the reference's own loops on the device (k_step_serial)
    // ... unless every goal is told to stand still (the zero move): such a call is an ordinary one -- one small launch and one read-back
    // decide it, against about a microsecond per list entry of the whole world on the literal loop's single lane
    bool goals_act = G.type->can_absorb && G.n > 0 && !G.acted && !serial_calls_on;     // (an empty group of goals moves nobody)
    if (goals_act) {
        enter();
        int *flag = d_counters + CTR_GOALS_ACT;
        HIP_OK(hipMemsetAsync(flag, 0, sizeof(int), stream));
        launch_any_real_action(stream, d_act, G.n, G.tdev, d_delta, flag);
        int h_flag = 0;
        read_back(&h_flag, flag, sizeof(int));
        goals_act = h_flag != 0;
        static std::atomic<bool> told{false};      // (set_action_device runs on env_cycle_many's worker threads too)
        if (goals_act && !told.exchange(true, std::memory_order_relaxed)) {
            std::fprintf(stderr, "magent-amd: a group of goals (can_absorb) was given actions that move, turn or attack: such steps run the reference's "
                                 "sequential loops on one lane of the device -- exact, about a microsecond per action of the whole world (INTEGRATION.md)\n");
        }
    }
    if (G.acted || serial_calls_on || goals_act) {
        serial_add_call(g, d_act);
        G.acted = true;
        return;
    }
    G.acted = true;
    if (step_calls.empty()) {           // the first call of a step fixes the form of all of them: worlds that step in one launch take the
        step_sa_tiled = !solo_ok(total_agents());   // one-workgroup form (sequence numbers assigned at once), the others leave tile counts (SeqPlan)
        sa_tiles = 0;
    }
    step_calls.push_back(g);
    if (G.n == 0) return;
    int base = 0;
    const int off = G.sa_off = count_action_call(G, &base);
    if ((size_t)sa_tiles > asums_cap) {      // (the counts of the step's earlier calls are kept)
        enter();
        grow(arena, d_asums, asums_cap, (size_t)sa_tiles, stream, true, (size_t)off);
        grow(arena, d_wpre, wpre_cap, asums_cap * (SCAN_TILE_HOST / 64), stream, true, (size_t)off * (SCAN_TILE_HOST / 64));
    }
    hipStream_t s = action_stream();    // large worlds: beside the observation renders (see side_stream)
    ProfScope p(*this, "set_action", false, s);
    launch_set_action(s, view(), g, d_act, base, d_asums, d_wpre, off);
}

// The accounting of one set_action call for G.n > 0 agents (set_action_device; Env::pipe_prepare for the batched pipeline): its order keys
// start at *base (a 27-bit insertion index, step.hip claim_word); in the tiled form its tile counts go to the returned offset of d_asums
// (-1: the one-workgroup form).  Growing d_asums / d_wpre stays with the callers: call by call, or once for all calls of a batch item.
int Env::count_action_call(const HostGroup &G, int *base) {
    if ((long long)move_seq_base + G.n >= (1ll << 27)) fatal("more than 2^27 agents given actions in one step");
    *base = move_seq_base;
    move_seq_base += G.n;
    if (!step_sa_tiled) return -1;
    const int off = sa_tiles;
    sa_tiles += (G.n + SCAN_TILE_HOST - 1) / SCAN_TILE_HOST;
    return off;
}

// Repeated set_action inside one step.  From the first repetition on every call of the step is kept as a list of (group, saved copy
// of the actions) in call order -- the earlier calls' actions are recovered from the pending actions they left -- and the step runs
// the reference's sequential loops on the device (k_step_serial).
void Env::serial_add_call(int g, const int *d_act) {
    enter();
    auto keep = [&](int gg, const int *src, bool from_pend) {
        HostGroup &G = groups[gg];
        int *buf = nullptr;
        if (G.n > 0) {
            HIP_OK(dev_malloc(arena, &buf, sizeof(int) * (size_t)G.n));
            GroupDev D = G.cur; D.n = G.n;
            if (from_pend) launch_pend_to_actions(stream, D, G.tdev, buf);
            else HIP_OK(hipMemcpyAsync(buf, src, sizeof(int) * (size_t)G.n, hipMemcpyDeviceToDevice, stream));
            // Agent::set_action stores last_action at once (GridWorld.h:176-178): an observation asked for before the step shows the latest call
            HIP_OK(hipMemcpyAsync(G.cur.last_action, buf, sizeof(int) * (size_t)G.n, hipMemcpyDeviceToDevice, stream));
        }
        serial_calls.push_back({gg, buf});
    };
    if (!serial_calls_on) {
        serial_calls_on = true;
        for (int gg : step_calls) keep(gg, nullptr, true);
    }
    keep(g, d_act, false);
}

// ---------------- some group was given actions more than once: the reference's sequential loops, on the device
void Env::serial_step() {
    scratch_for(Scratch::Other);
    step_kind = StepKind::Serial;            // (reports through the pinned record like the single-sync driver)
    step_live_paint = live_paint_now = false;   // the painted map is rebuilt by the next observation
    WorldView W = view();
    size_t entries = 0;
    for (auto &c : serial_calls) entries += (size_t)groups[c.g].n;
    // (the lists' scratch is kept from one such step to the next; the attack events share the array of the checked driver's)
    grow(arena, d_events, events_cap, entries + 1, stream);
    grow(arena, serial_alist, serial_alist_cap, entries + 1, stream);
    grow(arena, serial_mlist, serial_mlist_cap, 2 * (entries + 1), stream);
    grow(arena, serial_dcalls, serial_dcalls_cap, serial_calls.size(), stream);
    int2 *alist = serial_alist; int4 *mlist = serial_mlist, *msorted = serial_mlist + (entries + 1), *events = d_events; SerialCall *d_calls = serial_dcalls;
    HIP_OK(hipMemcpyAsync(d_calls, serial_calls.data(), sizeof(SerialCall) * serial_calls.size(), hipMemcpyHostToDevice, stream));
    const int n_sep = large_map_mode ? (width + bandwidth - 1) / bandwidth : 0;
    if (n_sep >= 39) fatal("internal: too many move stripes for the serial step");
    push_rng();
    launch_step_serial(stream, W, d_calls, (int)serial_calls.size(), alist, mlist, msorted, n_sep, events);
    rules_launch(W);
    launch_step_report(stream, d_counters, h_rec, ++step_seq, (int)groups.size());
    HIP_OK(hipStreamSynchronize(stream));    // (the slow path: the scratch goes back at once)
    if (!first_render) record_attack_events(events, read_counters()[CTR_LAST_A]);
    for (auto &c : serial_calls) if (c.actions) { int *buf = const_cast<int *>(c.actions); dfree(arena, buf); }
    serial_calls.clear();
    serial_calls_on = false;
}

// the attack events of the step for the text render: recorded once rendering has started (GridWorld.cc:484,508)
void Env::record_attack_events(const int4 *events, int n) {
    std::vector<int4> ev((size_t)std::max(n, 0));
    if (n > 0) read_back(ev.data(), events, sizeof(int4) * (size_t)n);
    attack_events.clear();
    for (const int4 &e : ev) if (e.w) attack_events.push_back({e.x, e.y, e.z});
}

void Env::set_action_host(int g, const int *actions) {
    if (g < 0 || g >= (int)groups.size()) fatal("invalid group handle in set_action : %d", g);
    use_device();
    HostGroup &G = groups[g];
    hipStream_t s = stream;
    if (G.n > 0) {
        if ((size_t)G.n > actions_cap) { enter(); grow(arena, d_actions, actions_cap, (size_t)G.n, stream); }
        s = action_stream();
        HIP_OK(hipMemcpyAsync(d_actions, actions, sizeof(int) * G.n, hipMemcpyHostToDevice, s));
    }
    set_action_device(g, d_actions);
    HIP_OK(hipStreamSynchronize(s));   // d_actions is reused by the next call
}

// ------------------------------------------------------------------------------------------------ step
// GridWorld::step (GridWorld.cc:456-631).
//
// Two drivers over the same kernels:
//   * single-sync (default): every phase is enqueued without waiting for the device.  The attack list length and the
//     engine RNG state are read on the device; the fixed-point rounds of the attack and move phases are launched
//     optimistically (`opt_attack_pairs` pairs, `opt_move_batches` batches) and gated on the device -- a round
//     returns at once when its phase has converged.  ONE readback at the end returns `done`, the death counts, the
//     RNG state and whether a phase ran out of rounds; in that (rare) case everything after that phase has been
//     skipped on the device and the host continues from exactly that state with the checked driver.
//   * checked: the host reads the convergence flag after every pair / batch (also used while the text render is
//     recording attack events, and with MAGENT_TUNE host_shuffle=1 / checked_step=1 for A/B runs).
void Env::shuffle_buffers(int n_max) {
    grow(arena, d_rank, rank_cap, (size_t)n_max, stream);
    if ((size_t)n_max * 4 > shuf_cap) {   // four arrays: head | first | j | link
        grow(arena, d_shuf, shuf_cap, (size_t)n_max * 4, stream);
        shuf_cap -= shuf_cap % 4;
        // head and first are kept zero between steps (k_attack_rank clears what a step used)
        HIP_OK(hipMemsetAsync(d_shuf, 0, sizeof(int) * shuf_cap, stream));
    }
    int nb = (n_max + SCAN_TILE_HOST - 1) / SCAN_TILE_HOST;
    grow(arena, d_sums, sums_cap, (size_t)nb, stream);
    // powers of the minstd_rand0 multiplier for k_shuffle_draw: 16807^t (t < 256), then 16807^(256 h) up to h = n_max / 256 + 1
    const size_t need = 256 + (size_t)n_max / 256 + 2;
    if (need > powtab_cap) {
        grow(arena, d_powtab, powtab_cap, need, stream);
        std::vector<unsigned> tab(powtab_cap);
        const unsigned long long P = 2147483647ull;
        tab[0] = 1;
        for (int t = 1; t < 256; t++) tab[t] = (unsigned)(tab[t - 1] * 16807ull % P);
        const unsigned long long step = tab[255] * 16807ull % P;
        tab[256] = 1;
        for (size_t h = 257; h < powtab_cap; h++) tab[h] = (unsigned)(tab[h - 1] * step % P);
        HIP_OK(hipMemcpy(d_powtab, tab.data(), sizeof(unsigned) * powtab_cap, hipMemcpyHostToDevice));
    }
}

ShuffleBufs Env::shuffle_bufs() const {
    const size_t seg = shuf_cap / 4;
    return ShuffleBufs{d_shuf, d_shuf + seg, d_shuf + 2 * seg, d_shuf + 3 * seg};
}

void Env::push_rng() {
    if (rng_on_device) return;
    launch_set_rng(stream, d_counters, (unsigned)rng.x);
    rng_on_device = true;
}

// move preparation (starve / recover first) / move apply / rules and the generic bodies' finish, for this world's kind of body
void Env::move_prep(const WorldView &W, bool starve) {
    if (any_multicell) launch_movg_prep(stream, W, starve); else launch_move_prep(stream, W, d_gtab);
}

void Env::move_apply(const WorldView &W) {
    if (any_multicell) launch_movg_apply(stream, W, d_gtab); else launch_move_apply(stream, W, d_gtab);
}

void Env::rules_launch(const WorldView &W) {
    if (!rules_on_host) launch_rules(stream, W, rule_args.data(), (int)rule_args.size(), rule_progs.data(), d_gtab);
}

void Env::rules_and_finish(const WorldView &W) {
    rules_launch(W);
    if (any_multicell) launch_finish(stream, W);   // (the 1x1 move commit already consumed the pending actions)
}

// attack rounds, host-checked: pairs with ONE convergence check per pair (the flag of the second round)
void Env::attack_rounds_checked(const WorldView &W) {
    const bool plain = step_kind == StepKind::Pipeline;     // (the continuation of a step of the plain pipeline: its own rounds)
    const PlainWorld PW = plain ? plain_view() : PlainWorld{};
    int iters = 0;
    while (true) {
        clear_changed();
        for (int flag : {-1, CTR_CHANGED}) {
            if (plain) launch_plain_eval(stream, W, PW, d_ptab, d_gtab, d_ttab, ++attack_round, flag, shuffle_bufs());
            else launch_attack_iter(stream, W, d_gtab, d_ttab, ++attack_round, attack_kmax, flag);
        }
        iters += 2;
        if (!read_changed()) break;
        if (iters > 1000000) fatal("attack resolution did not converge");
    }
    last_attack_iters = iters;
}

// move rounds, host-checked: `move_jump_batch` rounds per convergence check (a resolved agent is a no-op later)
void Env::move_rounds_checked(const WorldView &W) {
    if (!any_multicell) { last_move_iters = 0; return; }   // one-cell bodies: the commit walks the dependency chains itself (move_resolve)
    int iters = 0;
    do {
        clear_changed();
        for (int k = 0; k < move_jump_batch; k++) {
            const int flag = k == move_jump_batch - 1 ? CTR_CHANGED : -1;
            launch_movg_sweep(stream, W, d_gtab, flag);
        }
        iters += move_jump_batch;
        if (iters > 1000000) fatal("move resolution did not converge");
    } while (read_changed());
    last_move_iters = iters;
}

void Env::phase_tail(const WorldView &W, int from /* 0 = after attack rounds, 1 = after move rounds */) {
    if (step_kind == StepKind::Pipeline) {             // (only its attack rounds can run out: from == 0)
        launch_plain_tail(stream, W, plain_view(), d_ptab, d_gtab, d_ttab, step_fused_rules ? rule_args.data() : nullptr, (int)rule_args.size(), nullptr, 0);
        if (!step_fused_rules) rules_launch(W);
        return;
    }
    if (from == 0) {
        launch_attack_apply(stream, W, d_gtab, d_ttab, attack_kmax);
        move_prep(W);
        move_rounds_checked(W);
    }
    move_apply(W);
    rules_and_finish(W);
}

// The per-cell scratch words (claim, hitbits) as the three step paths want them and leave them:
//   one-launch step / cycle (Solo): wants every claim word CLAIM_NONE and every hit word zero; keeps them so
//   step of plain games (Plain): does not use the hit words (its hits live in per-agent masks); its claim words carry the epoch of the step
//       that wrote them (step.hip: claim_word) and are never cleaned -- it wants every word either filled (all ones) or written by a
//       plain step of the current window of 63 epochs, so the array is refilled when a window begins and after any other path wrote it
//   everything else (Other): wants nothing (fills what it needs) and leaves both arrays dirty
void Env::scratch_for(Scratch path) {
    const size_t ncell = (size_t)width * height;
    if (path == Scratch::Other) { claim_clean = claim_epochs = hit_clean = false; return; }
    if (path == Scratch::Solo && !hit_clean) { HIP_OK(hipMemsetAsync(d_hit, 0, sizeof(unsigned) * ncell, stream)); hit_clean = true; }
    if (path == Scratch::Plain) {
        plain_epoch++;
        if (plain_epoch % 63u == 0) claim_epochs = false;      // a new window: the oldest words would look like this step's
    }
    if (!claim_clean && !(path == Scratch::Plain && claim_epochs)) {
        HIP_OK(hipMemsetAsync(d_claim, 0xFF, sizeof(unsigned long long) * ncell, stream));
        claim_clean = true;
        if (path == Scratch::Plain) claim_refills++;
    }
    if (path == Scratch::Solo) claim_epochs = true;    // (filled is a special case of "filled or written in this window")
    else { claim_clean = false; claim_epochs = true; }
}

void Env::step(int *done) {
    step_begin();
    step_end(done);
}

// Worlds of up to `solo_max_agents` agents step in ONE launch (k_step_solo).  Not taken: food_mode (its per-cell food
// evaluation sweeps the map), hit lists that do not fit one workgroup's LDS, the A/B drivers, and steps that record attack
// events for the text render.
// Two limits (measured on the MI355X, profiles/r05_summary.md "one workgroup or a dozen launches"): an environment stepping on its own
// is faster through the multi-launch pipeline from ~1500 agents on in battle (2 x 1200: 0.093 ms per cycle against 0.141; 2 x 2000:
// 0.090 against 0.138; 2 x 8000: 0.109 against 0.389 -- one workgroup is one CU of 256) and level with it below; games with fewer
// fighters per agent (gather, pursuit) cross over later, at 2500-3000, and lose 0.015 ms per cycle to the lower limit there.  An
// environment that is one of a batch (env_cycle_many: one workgroup per environment, all in one launch) keeps the one-launch step up
// to 16384 agents -- the other CUs are busy with the other environments.
bool Env::solo_ok(int total_n) {
    return solo_enabled && !checked_step && !host_shuffle && !opt_fixed && first_render && !food_mode && !rules_on_host && total_n > 0 &&
           total_n <= (batch_width > 1 ? batch_solo_max : solo_max_agents) && solo_nt_eval >= 64;
}

// the host side of k_step_solo's report: spin on the sequence number in pinned memory
void Env::wait_record(int seq) {
    spin_until([&] { return h_rec->seq == seq; }, stream, "the one-launch step finished without publishing its record", "step kernel");
    std::atomic_thread_fence(std::memory_order_acquire);
}

void Env::enqueue_counters() {
    HIP_OK(hipMemcpyAsync(h_counters, d_counters, sizeof(int) * CTR_TOTAL, hipMemcpyDeviceToHost, stream));
}

// everything of the step that needs no answer from the device (single-sync driver), or the whole host-checked step: the common head and
// tail of the four drivers -- serial_step, solo_step, single_sync_step (over plain_step_tail or generic_step_tail), checked_step_run
void Env::step_begin() {
    if (!device_ready) fatal("step called before reset");
    if (step_pending) fatal("step_begin called twice without step_end");
    use_device();
    if (!tables_valid) { ensure_tables(); state_epoch++; }   // (enqueued on `stream`: the side stream has to see it)
    step_live_paint = live_paint_now = paint_valid;   // the painted map is current: every driver of the step keeps it so
    move_nodes();
    WorldView W = view();
    const int total_n = total_agents();
    // (turn_mode with generic bodies: a third fixed point -- the turns -- between starvation and the moves; it runs under the
    // host-checked driver, or inside the one-launch step)
    const bool generic_turns = turn_mode && any_multicell;
    const bool fast = !checked_step && !host_shuffle && first_render && !generic_turns;
    step_pending = true;
    alive_valid = false;
    map_warm = false;
    step_kind = StepKind::None;

    const bool beside = total_n > 0 && fast && side_wanted() && overlap_level >= 2 && !serial_calls_on;   // the read-only head of the step goes beside the renders
    if (!beside) join_side();
    step_calls.clear();
    if (total_n == 0) {
        enqueue_counters();
    } else if (serial_calls_on) {
        serial_step();
    } else if (solo_ok(total_n)) {
        solo_step(W, total_n);
    } else if (fast) {
        if (!single_sync_step(W, total_n, beside)) launch_step_report(stream, d_counters, h_rec, ++step_seq, (int)groups.size());
    } else {
        checked_step_run(W, total_n, generic_turns);
    }
    stale_events = true;      // (last_op / op_obj hold this step's events until clear_dead resets them)
    for (auto &g : groups) g.sa_off = -1;
    state_epoch++;
}

// groups that were given their actions in tiles (the world was beyond the one-launch step's limit at the time of the call, or is one of a
// batch now): the sequence numbers, and the attack list's length, are written out ahead of a one-launch step
void Env::assign_pending_seq(const WorldView &W) {
    bool first = true;
    for (size_t g = 0; g < groups.size(); g++)
        if (groups[g].sa_off >= 0) { launch_seq_assign(stream, W, (int)g, d_asums, d_wpre, groups[g].sa_off, first); first = false; }
}

// what the one-launch step and the two-launch cycle tell k_step_solo alike (Env::cycle_prepare adds the cycle's own fields)
SoloStep Env::solo_step_args() {
    const ShuffleBufs B = shuffle_bufs();
    SoloStep S{};
    S.shead = B.head; S.sfirst = B.first; S.sj = B.j; S.slink = B.link;
    S.rank = d_rank; S.powtab = d_powtab; S.hit = d_hit;
    S.rules = d_rule_args; S.progs = d_rule_progs; S.n_rules = (int)rule_args.size();
    S.kmax = attack_kmax; S.nt_eval = solo_nt_eval; S.max_rounds = 1 << 20;
    S.rec = h_rec; S.seq = ++step_seq;
    return S;
}

// ---------------- one launch for the whole step
void Env::solo_step(const WorldView &W, int total_n) {
    step_kind = StepKind::Solo;
    shuffle_buffers(total_n);
    push_rng();
    scratch_for(Scratch::Solo);        // (fills after a multi-launch step or a reset: once)
    assign_pending_seq(W);
    const SoloStep S = solo_step_args();
    ProfScope p(*this, "step");
    launch_step_solo(stream, W, S);
}

// ---------------- single-sync driver: the attack phase up to its optimistic rounds, then the tail of the world's kind.  Returns whether
// the step's report has gone out already (the plain pipeline with fused rules sends it ahead of the moves)
bool Env::single_sync_step(const WorldView &W, int total_n, bool beside) {
    const bool plain = W.plain != 0;       // plain games have a pipeline of their own behind the shuffle (step.hip: k_plain_rank ...)
    step_kind = plain ? StepKind::Pipeline : StepKind::Generic;
    if (plain) plain_steps++;
    scratch_for(plain ? Scratch::Plain : Scratch::Other);
    PlainWorld PW{};
    if (plain) PW = plain_view();
    {
        const size_t caps = rank_cap + shuf_cap + sums_cap + powtab_cap;
        const bool rng_here = !rng_on_device;
        shuffle_buffers(total_n);
        push_rng();
        if (rng_here || caps != rank_cap + shuf_cap + sums_cap + powtab_cap) state_epoch++;   // (something was enqueued on `stream`)
    }
    // shuffle, hit gather and the death-rank fixed point only read the world (and write scratch no render looks at)
    hipStream_t a = beside ? side_stream() : stream;
    {
        ProfScope p(*this, "attack", false, a);
        // (plain games keep their hits in per-agent masks; otherwise the draw zero-fills the per-cell hit words)
        if (plain) launch_shuffle_draw(a, total_n, d_counters, shuffle_bufs(), d_powtab, step_sa_tiled);
        else launch_shuffle(a, total_n, d_counters, shuffle_bufs(), d_rank, d_hit, (size_t)width * height, d_powtab, step_sa_tiled);
        if (overlap_level == 2 && a != stream) { join_side(); a = stream; }
        attack_round = 0;
        const int pairs = opt_fixed ? opt_attack_pairs : (boost_attack > 0 ? 2 : 1);
        if (plain) { if (pairs >= 2) pairs_two_steps++; else if (pairs == 1) pairs_one_steps++; }
        // rounds after the first only touch agents whose inputs changed: they are launched back to back and the
        // LAST one reports whether anything still moved (one gate for all of them)
        if (plain) launch_plain_rank(a, W, PW, d_ptab, shuffle_bufs(), d_asums, d_wpre, seq_plan());
        else launch_attack_rank(a, W, d_gtab, d_rank, shuffle_bufs(), false, d_asums, d_wpre, seq_plan());
        for (int r = 0; r < 2 * pairs; r++) {
            const int flag = r == 2 * pairs - 1 ? CTR_OPEN_ATTACK : -1;
            if (plain) launch_plain_eval(a, W, PW, d_ptab, d_gtab, d_ttab, ++attack_round, flag, shuffle_bufs());
            else launch_attack_iter(a, W, d_gtab, d_ttab, ++attack_round, attack_kmax, flag);
        }
        if (pairs == 0) launch_set_counter(a, d_counters, CTR_OPEN_ATTACK, 1, -1);   // tests: straight to the host
    }
    join_side();      // from here on the world changes: behind every render enqueued so far
    if (!plain) { generic_step_tail(W); return false; }
    return plain_step_tail(W, PW);
}

// k_strike and the moves of a plain world.  Returns whether the report went out with them
bool Env::plain_step_tail(const WorldView &W, const PlainWorld &PW) {
    const bool fuse = step_fused_rules = !rules_on_host && !stale_events && fused_rules(rule_args.data(), (int)rule_args.size());
    // (with the rules fused -- or none -- nothing the report carries is decided behind k_strike: it goes out before the moves)
    static const bool early = tune("early_report", 1) != 0;          // (MAGENT_TUNE early_report=0: behind the moves, for A/B runs)
    const bool reported = fuse && early;
    {
        ProfScope p(*this, "move");
        launch_plain_tail(stream, W, PW, d_ptab, d_gtab, d_ttab, fuse ? rule_args.data() : nullptr, (int)rule_args.size(),
                          reported ? h_rec : nullptr, reported ? ++step_seq : 0);
    }
    if (!fuse && !rules_on_host) {
        ProfScope p(*this, "rules");
        rules_launch(W);
    }
    alive_valid = true;
    return reported;
}

// attack apply, optimistic move rounds and the rules of every other world
void Env::generic_step_tail(const WorldView &W) {
    {
        ProfScope p(*this, "attack");
        launch_attack_apply(stream, W, d_gtab, d_ttab, attack_kmax);
    }
    {
        ProfScope p(*this, "move");
        move_prep(W);
        // (one-cell bodies need no rounds: the commit walks the dependency chains itself; the generic sweeps iterate)
        const int batches = opt_fixed ? opt_move_batches : (boost_move > 0 ? 2 : 1);
        for (int r = 0; any_multicell && r < batches * move_jump_batch; r++) {
            const int flag = r == batches * move_jump_batch - 1 ? CTR_OPEN_MOVE : -1;   // the last round reports
            launch_movg_sweep(stream, W, d_gtab, flag);
        }
        if (batches == 0) launch_set_counter(stream, d_counters, CTR_OPEN_MOVE, 1, CTR_OPEN_ATTACK);   // tests
        move_apply(W);
    }
    ProfScope p(*this, "rules");
    rules_and_finish(W);
}

// ---------------- checked driver: the host reads the convergence flag of every fixed point
void Env::checked_step_run(const WorldView &W, int total_n, bool generic_turns) {
    step_kind = StepKind::Checked;
    scratch_for(Scratch::Other);
    HIP_OK(hipMemsetAsync(d_counters + CTR_OPEN_ATTACK, 0, 2 * sizeof(int), stream));
    int A = read_counters()[CTR_ATTACK];
    if (step_sa_tiled) for (int k = 0; k < ATT_SLOTS; k++) A += h_counters[att_slot(k)];   // (the tiled set_action's spread counters: k_shuffle_draw adds them up too)
    if (A > 0) {
        ProfScope p(*this, "attack");
        shuffle_buffers(std::max(A, total_n));
        if (host_shuffle) {   // the reference's literal loop on the host (MAGENT_TUNE host_shuffle=1, for A/B checks)
            if (rng_on_device) { rng.x = (unsigned)read_counters()[CTR_RNG]; }
            if ((size_t)A > hrank_cap) {
                if (h_rank) HIP_OK(hipHostFree(h_rank));
                hrank_cap = std::max<size_t>((size_t)A, hrank_cap * 2);
                HIP_OK(hipHostMalloc((void **)&h_rank, sizeof(int) * hrank_cap, hipHostMallocDefault));
            }
            shuffle_perm.resize(A);
            for (int i = 0; i < A; i++) shuffle_perm[i] = i;
            for (int i = 0; i < A; i++) {
                int j = (int)rng() % (i + 1);
                std::swap(shuffle_perm[i], shuffle_perm[j]);
            }
            for (int pos = 0; pos < A; pos++) h_rank[shuffle_perm[pos]] = pos;
            HIP_OK(hipMemcpyAsync(d_rank, h_rank, sizeof(int) * A, hipMemcpyHostToDevice, stream));
            if (step_sa_tiled) launch_set_counter(stream, d_counters, CTR_ATTACK, A, -1);   // (k_shuffle_draw would have left the list's length there)
            rng_on_device = false;
        } else {              // exact parallel replay on the device
            push_rng();
            launch_shuffle(stream, total_n, d_counters, shuffle_bufs(), d_rank, d_hit, (size_t)width * height, d_powtab, step_sa_tiled);
        }
        launch_attack_rank(stream, W, d_gtab, d_rank, shuffle_bufs(), host_shuffle, d_asums, d_wpre, seq_plan());
        attack_round = 0;
        attack_rounds_checked(W);
        if (!first_render) {
            grow(arena, d_events, events_cap, (size_t)A, stream);
            launch_attack_events(stream, W, d_events);
            record_attack_events(d_events, A);
        }
        launch_attack_apply(stream, W, d_gtab, d_ttab, attack_kmax);
    } else if (!first_render) attack_events.clear();
    if (generic_turns) {
        ProfScope p(*this, "turn");
        launch_turn_prep(stream, W);        // (starvation first)
        int iters = 0;
        do {
            clear_changed();
            for (int k = 0; k < move_jump_batch; k++) launch_turn_sweep(stream, W, d_gtab, k == move_jump_batch - 1 ? CTR_CHANGED : -1);
            iters += move_jump_batch;
            if (iters > 1000000) fatal("turn resolution did not converge");
        } while (read_changed());
        launch_turn_apply(stream, W);
    }
    {
        ProfScope p(*this, "move");
        move_prep(W, !generic_turns);
        move_rounds_checked(W);
        move_apply(W);
    }
    {
        ProfScope p(*this, "rules");
        rules_and_finish(W);
    }
    enqueue_counters();
}

PlainWorld Env::plain_view() {
    PlainWorld PW{};
    for (size_t g = 0; g < groups.size(); g++) PW.g[g] = groups[g].pl;
    PW.S = plain_slots; PW.kmax = attack_kmax;
    {   // where k_strike leaves its survivor counts (one per 256 agents, group after group)
        size_t total = 0;
        for (size_t g = 0; g < groups.size(); g++) { alive_off[g] = (int)total; alive_n[g] = groups[g].n; total += (size_t)(groups[g].n + 255) / 256; }
        grow(arena, d_alive, alive_cap, std::max<size_t>(total, 1), stream);
        PW.alive = d_alive;
        for (int g = 0; g < MAXG; g++) PW.alive_off[g] = g < (int)groups.size() ? alive_off[g] : 0;
    }
    PW.epoch = 62 - (int)(plain_epoch % 63u);
    PW.round_base = (int)(plain_epoch * 64u);            // (wraps after 2^26 steps: the stamps are compared modulo 2^32)
    if (!ptab_valid) {
        if (!d_ptab) HIP_OK(dev_malloc(arena, &d_ptab, sizeof(PlainGroup) * MAXG));
        HIP_OK(hipMemcpyAsync(d_ptab, PW.g, sizeof(PlainGroup) * MAXG, hipMemcpyHostToDevice, stream));   // (pageable source: the copy is done when the call returns)
        ptab_valid = true;
        state_epoch++;
    }
    return PW;
}

SeqPlan Env::seq_plan() const {
    SeqPlan P{};
    for (int g = 0; g < MAXG; g++) P.off[g] = g < (int)groups.size() ? groups[g].sa_off : -1;
    return P;
}

// what a step reports (the deaths, the takings, the rules' triggers, the error flags, the generator), as a StepRecord made from the counter
// block: the deaths are spread over DEAD_SLOTS counters per group, every rule's trigger is a word (a phase that does not converge under the
// host's own rounds is fatal where it happens: no error code, no rounds)
StepRecord Env::record_of(const int *c) const {
    StepRecord r{};
    for (size_t g = 0; g < groups.size(); g++) {
        for (int k = 0; k < DEAD_SLOTS; k++) r.dead[g] += c[dead_slot((int)g, k)];
        r.taken[g] = c[CTR_TAKEN + g];
    }
    for (size_t k = 0; k < rules.size() && CTR_TRIGGER + (int)k < CTR_TRIGGER_END; k++) if (c[CTR_TRIGGER + k] != 0) r.triggers |= 1ull << k;
    r.rng = (unsigned)c[CTR_RNG];       // the device advanced the engine state by A draws
    r.unsupported = c[CTR_UNSUPPORTED]; r.pack_overflow = c[CTR_PACK_OVERFLOW]; r.bad_action = c[CTR_BAD_ACTION]; r.hit_overflow = c[CTR_HIT_OVERFLOW];
    return r;
}

// The end of every step, whichever driver ran it and whichever way it reported: the error flags, the generator, the death counts of the
// groups, `done`, the terminal rules -- and what the host knows about the device's state behind a step
void Env::finish_step(const StepRecord &O, int *done) {
    if (O.error) fatal("%s resolution did not converge", O.error == 1 ? "attack" : O.error == 2 ? "move" : "turn");
    if (O.unsupported) fatal("internal: a can_absorb agent moved on the parallel path (a set_action for goals switches the step to the literal loop)");
    if (O.pack_overflow) fatal("internal: hp / type.hp outside [0, 2) met the packed view-cell format");
    if (O.bad_action) fatal("set_action: an action outside [0, n_action) (the reference indexes its tables out of range here)");
    if (O.hit_overflow) fatal("a target collected more attack hits than the engine's hit lists hold (256)");
    if (rng_on_device) rng.x = O.rng;
    int live = 0;
    for (size_t g = 0; g < groups.size(); g++) {
        groups[g].h_dead = O.dead[g];
        groups[g].h_taken = O.taken[g];
        groups[g].acted = false;
        if (groups[g].n - groups[g].h_dead > 0) live++;
    }
    *done = live < (int)groups.size();   // GridWorld.cc:619-624
    for (size_t k = 0; k < rules.size(); k++)
        if ((rules_on_host ? host_triggers[k] != 0 : ((O.triggers >> k) & 1ull) != 0) && rules[k].terminal) *done = 1;
    move_seq_base = 0;
    h_occ_valid = false;
    paint_valid = step_live_paint; mini_valid = false;
    live_paint_now = false;
}

// the one host synchronisation of the step: `done`, death counts, RNG state, and the (rare) continuation when a
// phase ran out of optimistic rounds
void Env::step_end(int *done) {
    if (!step_pending) fatal("step_end without step_begin");
    step_pending = false;
    use_device();
    const bool by_record = reports_by_record(step_kind);   // the literal loop, the one-launch step and the single-sync driver
    if (by_record) {
        wait_record(step_seq);
        const StepRecord &r = *h_rec;
        if (!(r.open_attack | r.open_move)) {
            if (step_kind == StepKind::Solo) { last_attack_iters = r.rounds_attack; last_move_iters = r.rounds_move; attack_round = r.rounds_attack; }
            else {
                if (boost_attack > 0) boost_attack--;
                if (boost_move > 0) boost_move--;
                if (step_kind == StepKind::Pipeline) { int hi = 0; for (int b = 1; b < 32; b++) if ((r.rounds_mask >> b) & 1u) hi = b; round_hist[std::min(hi, 8)]++; }
            }
            if (rules_on_host) eval_rules_host();
            finish_step(r, done);
            return;
        }
        read_counters();     // a phase ran out of optimistic rounds: the whole counter block, for the continuation below
    }
    HIP_OK(hipStreamSynchronize(stream));
    const int *c = h_counters;
    if (by_record) {
        if (c[CTR_OPEN_ATTACK] | c[CTR_OPEN_MOVE]) {   // continue from exactly the device state the open phase froze, host-checked
            WorldView W = view();
            const int phase = c[CTR_OPEN_ATTACK] ? 1 : 2;
            fallback_steps++;
            if (phase == 1) fallback_attack++; else fallback_move++;
            // deeper dependency chains around: one more batch.  A step that runs out while the budget is ONE pair doubles the time the budget
            // stays at two from then on (64, 128, ... steps): in a dense world -- the bench's 2 x 400k at random: 8 run-outs in the 70 one-pair
            // steps of a 550-step episode, profiles/r06_raw/c3_episode_550_steps.txt -- a run-out (a host round trip and the host-checked rounds)
            // costs ten times what the second pair does; a sparse one (config 5's formation: 486 one-pair steps, none ran out) keeps the saving
            if (phase == 1) { if (boost_attack == 0) boost_window = std::min(boost_window * 2, 4096); boost_attack = boost_window; boost_ran_out = true; } else boost_move = 64;
            HIP_OK(hipMemsetAsync(d_counters + CTR_OPEN_ATTACK, 0, 2 * sizeof(int), stream));   // both phase flags
            clear_changed();
            if (phase == 1) { attack_rounds_checked(W); phase_tail(W, 0); }
            else { move_rounds_checked(W); phase_tail(W, 1); }
            c = read_counters();
        }
        if (boost_attack > 0) boost_attack--;
        if (boost_move > 0) boost_move--;
    }
    if (rules_on_host) eval_rules_host();
    finish_step(record_of(c), done);
    // attack count and rule triggers are per step; dead_ct lives until clear_dead
    launch_step_reset(stream, d_counters);
    HIP_OK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------ reward / clear_dead
void Env::get_reward_device(int g, float *out) {
    if (g < 0 || g >= (int)groups.size()) fatal("invalid group handle in get_reward : %d", g);
    enter();
    GroupDev G = groups[g].cur; G.n = groups[g].n;
    launch_get_reward(stream, G, groups[g].group_reward, out);
}

void Env::get_reward_host(int g, float *out) {
    if (g < 0 || g >= (int)groups.size()) fatal("invalid group handle in get_reward : %d", g);
    int n = groups[g].n;
    if (n == 0) return;
    grow(arena, d_stage_small, stage_small_cap, (size_t)n * 8, stream);
    get_reward_device(g, (float *)d_stage_small);
    read_back(out, d_stage_small, sizeof(float) * n);
}

// GridWorld::clear_dead (GridWorld.cc:633-665)
void Env::clear_dead() {
    if (!device_ready) fatal("clear_dead called before reset");
    enter();
    ProfScope p(*this, "clear_dead");
    WorldView W = view();
    bool any = false, all_solo = true, small_world = solo_enabled, next_mini = false;
    for (auto &G : groups) {
        if (G.h_dead + G.h_taken > 0) { any = true; all_solo &= compact_is_solo(G.n); }
        small_world &= compact_is_solo(G.n);
    }
    ClearArgs A{};
    for (size_t g = 0; g < groups.size(); g++) {
        const HostGroup &G = groups[g];
        A.mode[g] = G.n == 0 ? 0 : (G.h_dead + G.h_taken > 0 ? 2 : 1);
        A.dst[g] = G.alt_arrays();
    }
    if (small_world) {           // one launch of one workgroup: compaction / init_reward of every group + the device tables
        // the observations that follow will want the minimap of the window they used last: made here, by the same launch
        next_mini = minimap_mode && mini_vh > 0;
        MiniArgs M{};
        if (next_mini) M = mini_args(mini_vh, mini_vw, mini_skip);
        launch_clear_solo_all(stream, W, A, d_gtab, d_ttab, M);
        take_survivors();
        tables_valid = true;
    } else if (!any) {                  // Agent::init_reward for everybody: one launch (+ the normalisation of the next minimap)
        const MiniArgs M = next_minimap();
        launch_clear_compact(stream, W, A, d_sums, M, fold_counts());
        if (M.vh > 0) { launch_mini_norm(stream, W, M, fold_counts()); next_mini = true; }
    } else if (all_solo) {       // small worlds: one workgroup per group does everything for that group
        for (size_t g = 0; g < groups.size(); g++) {
            const HostGroup &G = groups[g];
            if (A.mode[g] == 2) {
                GroupDev D = G.cur;
                const AltArrays &T = A.dst[g];
                D.x = T.x; D.y = T.y; D.id = T.id; D.hp = T.hp; D.last_action = T.last_action;
                D.last_reward = T.last_reward; D.next_reward = T.next_reward; D.absorbed = T.absorbed; D.dir = T.dir;
                launch_compact(stream, W, (int)g, D, G.n - G.h_dead - G.h_taken, d_sums);
            } else {
                launch_init_reward(stream, W, (int)g);
            }
        }
        take_survivors();
        tables_valid = false;
    } else {                     // three launches for all groups together
        size_t nb_total = 0;
        for (size_t g = 0; g < groups.size(); g++) {
            A.sums_off[g] = (int)nb_total;
            nb_total += (groups[g].n + SCAN_TILE_HOST - 1) / SCAN_TILE_HOST;
        }
        grow(arena, d_sums, sums_cap, nb_total, stream);
        const MiniArgs M = next_minimap();
        // (the last step was one of the plain pipeline and nothing was added since: k_strike has left the survivors of every 256 agents)
        bool counted = alive_valid;
        for (size_t g = 0; g < groups.size(); g++) counted &= groups[g].n == alive_n[g];
        if (counted) {
            for (size_t g = 0; g < groups.size(); g++) A.sums_off[g] = alive_off[g];
            A.sums_per_tile = SCAN_TILE_HOST / 256;
        }
        launch_clear_compact(stream, W, A, counted ? d_alive : d_sums, M, fold_counts());
        take_survivors();
        launch_clear_finish(stream, view(), A, d_gtab, d_ttab, M, fold_counts());   // also refreshes the device tables
        tables_valid = true;
        next_mini = M.vh > 0;
    }
    after_clear(any, next_mini);
}

// the host's mirror of a compaction on the device: the groups that lost somebody (h_dead + h_taken, as the step reported them) find their
// survivors in the second copy of the double-buffered arrays; the rest was reset in place.  Returns whether there was such a group
bool Env::take_survivors() {
    bool any = false;
    for (auto &G : groups) if (G.n > 0 && G.h_dead + G.h_taken > 0) { G.take_survivors(); any = true; }
    return any;
}

// what the host knows behind a clear_dead, whichever launch ran it (Env::clear_dead, the two-launch cycle, the batched pipeline); next_mini:
// that launch also made the minimap of the next observations, for the window mini_vh x mini_vw / mini_skip
// (the death counters of the compacted groups were zeroed by the compaction kernels; the others were zero)
void Env::after_clear(bool any_compacted, bool next_mini) {
    for (auto &G : groups) {
        G.group_reward = 0;
        G.h_dead = G.h_taken = 0;
        G.indexed = G.n;                      // Agent::set_index (GridWorld.cc:655)
    }
    if (any_compacted) { h_occ_valid = false; mini_valid = false; }
    stale_events = false;
    alive_valid = false;                      // (k_strike's survivor counts describe the arrays as the step left them: consumed)
    if (next_mini) { mini_valid = true; mini_pop = mini_population(mini_skip); }
}

}  // namespace magent_amd
