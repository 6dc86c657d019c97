// pt_megakernel_loop.inc -- the launch loop of trace_paths_kernel (pt_megakernel.hip), included there THREE times: with PT_LOOP_QUAD 0 (one ray
// per lane) for the dense part of every launch (PT_LOOP_STAGE 0, PT_LOOP_FORK false) and again for a wavefront that has nothing left to start
// (PT_LOOP_STAGE 1, PT_LOOP_FORK true: shadow rays are handed to idle lanes), and with PT_LOOP_QUAD 1 (one ray per quad of lanes, once few paths
// are left; PT_LOOP_FORK = a launch parameter).  Textual instances rather than one loop with switches or a generic lambda: the first is then compiled
// exactly as if the others did not exist (registers, schedule), and the per-lane state stays in registers (a lambda that captures the
// kernel's other lambdas defeats the scalar replacement of the state struct: it ends up in scratch memory).
// Everything it names is a local of the kernel.
    constexpr bool quad = PT_LOOP_QUAD != 0;
    // read per instance of the loop, behind an opaque copy: carried from the first instance to the second this uniform flag was moved to a
    // vector register and spilled to scratch memory (the only scratch use of the kernel)
    uint32_t ref_mode = A.ref_mode;
    asm volatile("" : "+s"(ref_mode));
    for (;;) {
        // ------------------------------------------------------------------ shade DONE lanes
        {
            const unsigned long long m_done = __ballot(phase == kPhaseDone);
            const unsigned long long m_trav = __ballot(phase == kPhaseTrav);
            if (m_done != 0ull && ((uint32_t)__popcll(m_done) >= shade_due(m_trav | m_done) || m_trav == 0ull)) {
                if (TIMELINE) ++n_shade;
                if (STATS) cy_mark = __builtin_amdgcn_s_memtime();
                if (ref_mode) {
                    // PT_MODE_REFERENCE: every ray here is a camera ray that hit (a miss frees its lane without a shade pass and leaves
                    // the primed 0.01, renderer.wgsl:410); shade() of renderer.wgsl:348-353 with the stored geometric normal
                    if (phase == kPhaseDone) {
                        const F3 col = base * (0.15f + wmax(dot3(tri_normal_ref(A, S.best_tri), L), 0.0f));
                        A.samples[S.item] = make_float4(col.x, col.y, col.z, 1.0f);
                        phase = kPhaseIdle;
                    }
                } else {
                // Forked shadow rays (see the top of pt_megakernel.hip): a path that runs ahead of its shadow ray (kPendBit) looks at the seat (quad of lanes,
                // or lane) that traces it -- every lane, whatever its ray is doing; once that ray has ended its term goes into the path's radiance (the
                // path has added nothing since: it waits, kPhaseWait, at its next event that would) and the seat that traced it is free again.
                // One ray per lane: only once the wavefront has nothing left to start (idle lanes stay idle from then on).
                const bool fork_on = PT_LOOP_FORK;          // (a constant or a wave-uniform flag: see where this file is included)
                bool want_fork = false;
                if (fork_on) {
                    const int ca = (int)((S.bounce >> kChildShift) << 2);          // first lane of the seat that traces it, as a byte address (lane 0 when there is none)
                    const uint32_t c_phase = (uint32_t)__builtin_amdgcn_ds_bpermute(ca, (int)phase), c_tri = (uint32_t)__builtin_amdgcn_ds_bpermute(ca, (int)S.best_tri);
                    if (STATS) {
                        // the invariant nothing else enforces: a seat that ends a forked ray is read by its path in the very pass in which it goes idle (every
                        // lane's permute above precedes the phase changes below).  A path whose seat is idle, or no longer traces a forked ray, has lost
                        // a shadow term: bit 63 of counter word 7, checked by the tests.
                        const uint32_t c_bounce = (uint32_t)__builtin_amdgcn_ds_bpermute(ca, (int)S.bounce);
                        if ((S.bounce & kPendBit) && (c_phase == kPhaseIdle || (c_bounce & kForkedBit) == 0u)) atomicOr(&A.stats[7], 1ull << 63);
                    }
                    if ((S.bounce & kPendBit) && c_phase == kPhaseDone) {
                        if (c_tri == kInvalidRef) S.rad = S.rad + S.contrib;
                        S.bounce &= kFlagsMask;
                        if (phase == kPhaseWait) phase = kPhaseDone;
                    }
                    if (phase == kPhaseDone && (S.bounce & kForkedBit)) phase = kPhaseIdle;      // read by its path in this very pass
                    if (phase == kPhaseDone && (S.bounce & kPendBit)) { phase = kPhaseWait; if (STATS && count_lane()) ++n_fork_wait; }
                    __builtin_amdgcn_s_waitcnt(0xc07f);      // lgkmcnt(0), said here: otherwise the compiler carries "a permute may be pending" into the traversal loop and waits there, every step
                }
                bool finish = false, launch = false, next_bounce = false;      // next_bounce: the path goes on with its sampled direction (one site for the three reciprocals)
                const uint32_t bounce = S.bounce & 0xffffu;
                if (phase == kPhaseDone) {
                    const bool hit = S.best_tri != kInvalidRef;
                    if (S.bounce & kShadowBit) {
                        if (!hit) S.rad = S.rad + S.contrib;
                        if (S.bounce & kContBit) next_bounce = true;
                        else finish = true;
                    } else if (!hit) {
                        S.rad = S.rad + S.T * ((bounce == 0u) ? kBgPrimary : kSkyAmbient);
                        finish = true;
                    } else {
                        const F3 n = tri_normal_ref(A, S.best_tri);
                        // exposed triangles (pt_expose.hip): the word of the hit triangle's bit, asked for next to the normal (an independent load)
                        // (two tiers, their words interleaved: .x the first tier's, .y the second's -- one 8-byte load)
                        uint2 ex_word = make_uint2(0u, 0u);
                        uint32_t bx = A.bounces_expose;                // the bounce limit and the mask's place in one launch constant (pt_kernels.h)
                        asm volatile("" : "+s"(bx));                   // (opaque: what is derived from it is computed here, not hoisted out of the launch loops and held through them)
                        if ((bx >> 16) != 0u) ex_word = *(const uint2*)((const char*)A.scene + ((bx & 0xffff0000u) + (((S.best_tri & 0x7fffffffu) >> 7) << 3)));
                        // what does not depend on the normal is computed while it is on its way from memory (a dependent fetch the pass would otherwise sit out):
                        // the hit point, this bounce's random numbers, the direction sample in its local frame
                        const F3 hp = S.o + S.d * S.best_t;
                        const float u_rr = rnd(S.key, bounce, 4);
                        F3 l_next = cosine_local<BOUNDED>(rnd(S.key, bounce, 2), rnd(S.key, bounce, 3));
                        asm volatile("" : "+v"(l_next.x), "+v"(l_next.y), "+v"(l_next.z));       // (done HERE: before the first use of the normal)
                        const float nd = dot3(n, S.d);
                        const F3 nf = (nd < 0.0f) ? n : f3(-n.x, -n.y, -n.z);
                        const F3 so = hp + nf * kEpsOrigin;
                        const float ndl = dot3(nf, L);
                        S.contrib = (S.T * base) * ndl;
                        bool cont = bounce < (bx & 0xffffu);
                        if (cont) {
                            F3 Tn = S.T * base;
                            if (bounce >= kRRStart) {
                                const float p = wmax(wmax(Tn.x, Tn.y), Tn.z);
                                if (u_rr >= p) cont = false;
                                else Tn = Tn * rcp_f<BOUNDED>(p);
                            }
                            if (cont) { S.T = Tn; S.d_next = cosine_world<BOUNDED>(nf, l_next); }
                        }
                        S.o = so;
                        // The shadow ray of a hit on an exposed triangle finds nothing (DESIGN.md section 6.2: no triangle reaches into the prism its origin
                        // lies in, for hits at |n . d| >= the gate, which bounds the origin's error inside the plane): its term is added here -- where
                        // the traced ray's end would add it, nothing having been added in between -- and the path goes on as without a light term.
                        // The second tier's bit (a superset of the first's) says that the hit may be skipped at all, the first tier's which gate it has to pass.
                        // (the conditions are folded into one lane value and tested once: held as lane masks they cost spilled scalar registers)
                        const uint32_t ex_bit = (S.best_tri >> 2) & 31u;
                        uint32_t lit = (ex_word.y >> ex_bit) & 1u;
                        const float ex_gate = ((ex_word.x >> ex_bit) & 1u) != 0u ? kExposeGate : kExposeGate2;
                        lit = (fabsf(nd) >= ex_gate) ? lit : 0u;
                        lit = (ndl > 0.0f) ? lit : 0u;
                        asm volatile("" : "+v"(lit));
                        {   // (a select in front of the branch the pass had before, not a branch of its own: no further definition of the pass's lane masks)
                            const F3 r1 = S.rad + S.contrib;
                            S.rad = f3(lit != 0u ? r1.x : S.rad.x, lit != 0u ? r1.y : S.rad.y, lit != 0u ? r1.z : S.rad.z);
                            if (STATS && lit != 0u && count_lane()) ++c_lit;
                        }
                        if (ndl > 0.0f && lit == 0u) {
                            if (cont && fork_on) want_fork = true;          // settled below, with the other seats
                            else {
                            S.d = L; S.inv = invL;
                            S.bounce = bounce | kShadowBit | (cont ? kContBit : 0u);
                            launch = true;
                            }
                        } else if (cont) next_bounce = true;
                        else finish = true;
                    }
                }
                // A path that goes on after its shadow ray hands that ray to an idle seat of its wavefront and goes on AT ONCE (the k-th such
                // path takes the k-th idle seat that has a stack column); without an idle seat it traces the shadow ray itself, as before.
                uint32_t pend = 0u;
                if (fork_on) {
                    const unsigned long long m_fork = __ballot(want_fork);
                    if (m_fork != 0ull) {
                        const unsigned long long seats = quad ? 0x1111111111111111ull : ~0ull;          // the first lane of every seat
                        const uint32_t q0 = quad ? (lane & ~3u) : lane;
                        unsigned long long f = m_fork & seats, h = __ballot(phase == kPhaseIdle && (!quad || col != kNoCol)) & seats;
                        uint32_t my_child = 64u, my_path = 64u;
                        while (f != 0ull && h != 0ull) {
                            const uint32_t lf = (uint32_t)__builtin_ctzll(f), lh = (uint32_t)__builtin_ctzll(h);
                            f &= f - 1ull; h &= h - 1ull;
                            my_child = (q0 == lf) ? lh : my_child;
                            my_path = (q0 == lh) ? lf : my_path;
                        }
                        const int pa = (int)((my_path < 64u ? my_path : lane) << 2);
                        const float ox = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(pa, (int)__float_as_uint(S.o.x)));
                        const float oy = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(pa, (int)__float_as_uint(S.o.y)));
                        const float oz = __uint_as_float((uint32_t)__builtin_amdgcn_ds_bpermute(pa, (int)__float_as_uint(S.o.z)));
                        if (my_path < 64u) {                       // this seat takes a shadow ray: started below, like every other ray of this pass
                            S.o = f3(ox, oy, oz); S.d = L; S.inv = invL;
                            S.bounce = kShadowBit | kForkedBit;
                            phase = kPhaseDone; launch = true;
                            if (STATS) { path_steps = 0; path_shadow_steps = 0; }
                        }
                        if (want_fork) {
                            if (my_child < 64u) { pend = kPendBit | (my_child << kChildShift); next_bounce = true; if (STATS && count_lane()) ++n_fork; }
                            else { if (STATS && count_lane()) ++n_fork_none; S.d = L; S.inv = invL; S.bounce = bounce | kShadowBit | kContBit; launch = true; }
                        }
                        __builtin_amdgcn_s_waitcnt(0xc07f);  // (as above)
                    }
                }
                if (phase == kPhaseDone && (fork_on ? ((S.bounce & kForkedBit) == 0u || launch) : true)) {
                    if (next_bounce) { S.d = S.d_next; S.inv = safe_inv<BOUNDED>(S.d); S.bounce = (bounce + 1u) | pend; launch = true; }
                    if (launch) {
                        if (STATS) { if (count_lane()) { if (S.bounce & kShadowBit) ++c_shadow; else ++c_closest; } if (ray_steps > max_ray_steps) max_ray_steps = ray_steps; ray_steps = 0; }
                        phase = begin_ray() ? kPhaseTrav : kPhaseDone;   // a root miss is shaded on the next pass
                    }
                    if (finish) {
                        A.samples[S.item] = make_float4(S.rad.x, S.rad.y, S.rad.z, 1.0f);
                        phase = kPhaseIdle;
                        if (STATS) {
                            if (path_steps > max_path_steps) max_path_steps = path_steps;
                            if (queue_empty && path_steps > max_path_steps_post) max_path_steps_post = path_steps;
                            if (path_steps >= 512u && count_lane()) { ++long_paths; long_shadow_steps += path_shadow_steps; long_total_steps += path_steps; }
                            if (path_steps >= 1024u && count_lane()) ++longer_paths;
                        }
                    }
                }
                }
                if (STATS) cy_shade += __builtin_amdgcn_s_memtime() - cy_mark;
            }
        }
        // ------------------------------------------------------------------ time to re-seat the paths, one per quad of lanes?
        // (Asked HERE, behind the shade pass, not at the top of the loop: as the loop's first statement this exit made the register
        // allocator keep two copies of the whole lane state and move ~30 registers three times per pass -- 2 % of a dense frame.)
        if (!quad && PT_LOOP_STAGE == 0 && PT_FORK_LANES != 0 && A.fork_shadow >= 2u && source_dry()) { want_stage_b = true; break; }      // on with the loop's second one-ray-per-lane instance (shadow rays handed to idle lanes)
        if (PT_QUAD == 1 && !quad && A.quad_live != 0u && source_dry()) {
            const uint32_t n_live = (uint32_t)__popcll(__ballot(phase != kPhaseIdle));                // (a path that waits for its forked shadow ray is live)
            if (__builtin_expect(n_live != 0u && n_live <= A.quad_live, 0)) { want_reseat = true; break; }
        }
        // ------------------------------------------------------------------ refill IDLE lanes
        {
            const unsigned long long m_idle = __ballot(phase == kPhaseIdle);
            const unsigned long long m_trav = __ballot(phase == kPhaseTrav);
            if ((quad || PT_LOOP_STAGE == 0) && m_idle != 0ull && !source_dry() && ((uint32_t)__popcll(m_idle) >= A.fill_threshold || m_trav == 0ull)) {      // (the second one-ray-per-lane instance starts nothing)
                // quad mode (PT_QUAD == 2 only: a wavefront that re-seats its paths has nothing left to start): an idle quad takes one ray
                const uint32_t want = (uint32_t)__popcll(m_idle) >> (quad ? 2 : 0);
                const uint32_t rank = lanes_below(m_idle) >> (quad ? 2 : 0);
                if (TIMELINE) ++n_fill;
                if (STATS) cy_mark = __builtin_amdgcn_s_memtime();
                {
                    // Camera rays are GENERATED by the whole wavefront, one (frame, tile, sample) batch of 64 at a time -- item decode,
                    // RNG key, jittered ray, its rotation, the three correctly rounded reciprocals and the root-box test are ~300
                    // instructions whether 8 lanes need a ray or 64, so all 64 lanes compute (whatever their own ray is doing: only
                    // temporaries are touched), and the rays that enter the root box go, compacted, into the wavefront's ray buffer.
                    // Idle lanes then only FETCH a ready ray (three dwordx4).  A camera ray that misses the root box is never stored:
                    // its sample keeps the primed miss value (0 + 1 * 0.01, renderer.wgsl:410).
                    while (rb_next == rb_count && !queue_empty) {
                        if (chunk_next == chunk_end) claim_chunk();
                        if (queue_empty) break;
                        const uint32_t first = chunk_next; chunk_next += 64u;       // chunks are multiples of 64 items
                        const ItemInfo it = decode_item(A, first + lane);
                        bool enters = false; Ray r; uint32_t key = 0u;
                        r.o = r.d = r.inv = f3(0.0f, 0.0f, 0.0f);
                        if (it.valid) {
                            // every sample of the batch starts as the camera-ray miss value (0 + 1 * 0.01, renderer.wgsl:410); a path that
                            // hits something overwrites its own later (same wavefront, same address: in order).  Priming here, 64 lanes
                            // at a time, is what keeps the resolve pass read-only on the sample buffer.
                            // (the constant is made here, behind an opaque copy: hoisted out of the launch loop it occupies four registers
                            // through the traversal and ends up spilled to scratch memory)
                            float bgp = 0.0f + 1.0f * kBgPrimary;
                            asm volatile("" : "+v"(bgp));
                            A.samples[it.sample_index] = make_float4(bgp, bgp, bgp, 1.0f);
                            const FrameParams fp = frames[it.fid];
                            if (ref_mode) r = primary_ray_fp<BOUNDED>(A, fp, (float)it.px + 0.5f, (float)it.py + 0.5f);       // renderer.wgsl:387: the pixel centre
                            else {
                                key = sample_key(fp.seed, it.py * A.width + it.px, fp.frame * A.spp + it.s);
                                r = primary_ray_fp<BOUNDED>(A, fp, (float)it.px + rnd(key, 0, 0), (float)it.py + rnd(key, 0, 1));
                            }
                            if (STATS) { ++c_closest; ++c_samples; }
                            if (!scene_is_empty()) {
                                if (STATS) { c_nodes += 1; if (c_maxstack < 1u) c_maxstack = 1u; }   // the root record is fetched before its degenerate check (renderer.wgsl:240-244)
                                float troot;
                                if (A.root_degenerate == 0u) enters = slab(r, A.root_box[0], A.root_box[1], A.root_box[2], kInfT, troot);
                            }
                        }
                        const unsigned long long m_in = __ballot(enters);
                        if (STATS && enters) ++c_enter;
                        if (enters) {
                            uint4* rec = rb + (size_t)lanes_below(m_in) * 3;
                            rec[0] = make_uint4(__float_as_uint(r.o.x), __float_as_uint(r.o.y), __float_as_uint(r.o.z), __float_as_uint(r.d.x));
                            rec[1] = make_uint4(__float_as_uint(r.d.y), __float_as_uint(r.d.z), __float_as_uint(r.inv.x), __float_as_uint(r.inv.y));
                            rec[2] = make_uint4(__float_as_uint(r.inv.z), key, it.sample_index, 0u);
                        }
                        rb_count = (uint32_t)__popcll(m_in); rb_next = 0u;
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the records are written before any lane of this wavefront fetches one
                    }
                    const uint32_t avail = rb_count - rb_next;
                    if (phase == kPhaseIdle && rank < avail) {
                        const uint4* rec = rb + (size_t)(rb_next + rank) * 3;
                        const uint4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                        S.o = f3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z));
                        S.d = f3(__uint_as_float(r0.w), __uint_as_float(r1.x), __uint_as_float(r1.y));
                        S.inv = f3(__uint_as_float(r1.z), __uint_as_float(r1.w), __uint_as_float(r2.x));
                        S.key = r2.y; S.item = r2.z; S.bounce = 0u;
                        S.T = f3(1.0f, 1.0f, 1.0f); S.rad = f3(0.0f, 0.0f, 0.0f);
                        S.best_t = kInfT; S.best_tri = kInvalidRef; S.sp = 0; S.cur = A.root_ref; S.sel = ray_selectors(S.inv);
                        phase = kPhaseTrav;
                        if (STATS) { path_steps = 0; ray_steps = 0; path_shadow_steps = 0; }
                    }
                    rb_next += min(want, avail);
                }
                if (STATS) cy_fill += __builtin_amdgcn_s_memtime() - cy_mark;
            }
        }
        // ------------------------------------------------------------------ exit / idle-spin
        const unsigned long long m_trav = __ballot(phase == kPhaseTrav);
        if (m_trav == 0ull) {
            const unsigned long long m_done = __ballot(phase == kPhaseDone);
            if (m_done == 0ull && source_dry()) break;
            continue;
        }
        // ------------------------------------------------------------------ traversal steps, until one of the passes above is due again
        // (the lanes that traverse, as a wavefront mask: known from the test above and, after every step, from the pass conditions -- the step
        // takes it as its lane mask instead of comparing the phases once more)
        unsigned long long trav_now = m_trav;
        const uint32_t fill_thr = source_dry() ? 0x10000u : A.fill_threshold;       // (the source does not change inside the loops below; a dry one starts nothing)
#if !PT_LOOP_QUAD
        for (;;) {
        if (TIMELINE) { ++n_iter; lanes_sum += __popcll(trav_now); leaf_lanes += __popcll(trav_now & __ballot((S.cur & kLeaf) != 0u)); }      // wave-uniform: scalar counters
        if (STATS) { cy_mark = __builtin_amdgcn_s_memtime(); if (PT_LOOP_STAGE) { wait_seat_iters += __popcll(__ballot(phase == kPhaseWait)) >> (quad ? 2 : 0); live_seat_iters += __popcll(__ballot(phase != kPhaseIdle && !(S.bounce & kForkedBit))) >> (quad ? 2 : 0); } }
        if (lane_of(trav_now)) {
            bool need_pop = false;
            if (STATS) { ++path_steps; ++ray_steps; if (S.bounce & kShadowBit) ++path_shadow_steps; }
            // Unified fetch: a lane is either at an internal node (64 B record) or at a leaf (64 B triangle record).  Both kinds
            // live in one arena and a reference is the record's position in it (packed references, pt_host.h), so the same four
            // dwordx4 loads at `cur << 4` fetch either kind BEFORE the node/leaf branch: a wavefront with mixed lanes pays one
            // memory latency per step, not two.  (A leaf lane fetches its record's fourth piece, the normal, along with the three it tests.)
            // The pieces come back in the order they were asked for (the compiler asks for the fourth first) and nothing waits for all of them at once:
            // the node side runs FIRST and tests child 3, 2, 1, 0 -- each behind its own `s_waitcnt vmcnt(3..0)` --, the leaf side, which needs three
            // pieces before its first product, runs after it.  Two `if`s in this order, not if / else: the compiler runs the `cur < 0` side of an if / else
            // first whichever way it is written.
            const bool at_leaf = (S.cur & kLeaf) != 0u;
            const uint4* rec = arena_record(A, S.cur);
            uint4 n0 = rec[0], n1 = rec[1], n2 = rec[2], n3 = rec[3];
            if (!at_leaf) {
                float t0, t1, t2, t3;
                // all four slab tests are evaluated unconditionally: one 64 B fetch, no per-child branches or dependent
                // waits.  Empty slots and degenerate children (kDegenerateRef: counted below, never entered) hold the inverted
                // box, which slab_sel rejects by itself
                // child-major record (pt_host.h::WideNode): piece k = child k's box words + its reference
                const unsigned long long H3 = slab_sel(S.o, S.inv, S.sel, n3.x, n3.y, n3.z, S.best_t, t3);      // (in the order the pieces arrive)
                const unsigned long long H2 = slab_sel(S.o, S.inv, S.sel, n2.x, n2.y, n2.z, S.best_t, t2);
                const unsigned long long H1 = slab_sel(S.o, S.inv, S.sel, n1.x, n1.y, n1.z, S.best_t, t1);
                const unsigned long long H0 = slab_sel(S.o, S.inv, S.sel, n0.x, n0.y, n0.z, S.best_t, t0);
                const uint32_t r0 = n0.w, r1 = n1.w, r2 = n2.w, r3 = n3.w;
                if (STATS) c_nodes += (r0 != kInvalidRef) + (r1 != kInvalidRef) + (r2 != kInvalidRef) + (r3 != kInvalidRef);
                // Branch-free form of renderer.wgsl:314-342 for one lane.  Hit children keep slot order;
                // the nearest (first minimum of tmin) is entered next and trades places with the first
                // hit, so the stacked entry for slot s is the first hit's when s is the nearest slot, the
                // slot's own child otherwise -- and a slot is stacked iff it is hit and is not the first hit.
                // All predicates are wavefront masks: their logic runs on the scalar unit, the vector unit only selects.
                const float kBig = 3.0e38f;
                const float e0 = lane_of(H0) ? t0 : kBig, e1 = lane_of(H1) ? t1 : kBig, e2 = lane_of(H2) ? t2 : kBig, e3 = lane_of(H3) ? t3 : kBig;
                // nearest slot = first slot (in slot order) at the minimum, as a two-level tournament: the lower slot wins a tie at either level, which is "the first
                // minimum".  The same eight vector instructions as a four-way minimum + three equality tests + a chain of three selects, but only four of them
                // deep -- the nearest child's reference is what the NEXT step's fetch waits for.
                const unsigned long long C01 = __builtin_amdgcn_ballot_w64(e0 <= e1), C23 = __builtin_amdgcn_ballot_w64(e2 <= e3);
                const float m01 = min_f32(e0, e1), m23 = min_f32(e2, e3);
                const unsigned long long CL = __builtin_amdgcn_ballot_w64(m01 <= m23);
                const unsigned long long M1 = CL & ~C01, M2 = ~CL & C23, M3 = ~(CL | C23);
                const uint32_t rn01 = lane_of(C01) ? r0 : r1, rn23 = lane_of(C23) ? r2 : r3;
                const uint32_t rn = lane_of(CL) ? rn01 : rn23;
                if (lane_of(H0 | H1 | H2 | H3)) {
                    // slot s (1..3) is stacked iff it is hit and an earlier slot is hit too (so it is not the first hit); the first hit
                    // among the slots before s is then what the nearest slot hands over
                    const unsigned long long P3 = H3 & (H0 | H1 | H2), P2 = H2 & (H0 | H1), P1 = H1 & H0;
                    const float tf01 = lane_of(H0) ? t0 : t1; const uint32_t rf01 = lane_of(H0) ? r0 : r1;                         // first hit of slots 0..1 (when there is one)
                    const float tf012 = lane_of(H0 | H1) ? tf01 : t2; const uint32_t rf012 = lane_of(H0 | H1) ? rf01 : r2;       // first hit of slots 0..2
                    const unsigned long long w3 = ((unsigned long long)__float_as_uint(lane_of(M3) ? tf012 : t3) << 32) | (lane_of(M3) ? rf012 : r3);
                    const unsigned long long w2 = ((unsigned long long)__float_as_uint(lane_of(M2) ? tf01 : t2) << 32) | (lane_of(M2) ? rf01 : r2);
                    const unsigned long long w1 = ((unsigned long long)__float_as_uint(lane_of(M1) ? t0 : t1) << 32) | (lane_of(M1) ? r0 : r1);
                    if (__builtin_expect(S.sp + 3 <= kShort, 1)) {
                        // fast path: three unconditional LDS stores far -> near; an entry that is not
                        // stacked is simply overwritten by the next one (the slot index does not advance)
                        int sp1, sp2;
                        const int sp0 = S.sp;
                        unsigned long long* const slot0 = stk + sp0 * 64;
                        add_lane_bits3(S.sp, P3, P2, P1, sp1, sp2);
                        *slot0 = w3; stk[sp1 * 64] = w2; stk[sp2 * 64] = w1;
                        if (STATS) { const int k = S.sp - sp0; push_ops += k; for (int j = sp0; j < S.sp; ++j) { if (j >= 8) ++push8_ops; if (j >= 12) ++push12_ops; } }
                        if (STATS) { const uint32_t depth = (uint32_t)S.sp + 1u; if (depth > c_maxstack) c_maxstack = depth; }   // entries incl. the nearest child
                        S.cur = rn;
                    } else {
                        if (lane_of(P3)) push((uint32_t)w3, __uint_as_float((uint32_t)(w3 >> 32)));
                        if (lane_of(P2)) push((uint32_t)w2, __uint_as_float((uint32_t)(w2 >> 32)));
                        if (lane_of(P1)) push((uint32_t)w1, __uint_as_float((uint32_t)(w1 >> 32)));
                        if (STATS) { const uint32_t depth = (uint32_t)S.sp + (S.sp < kStackMax ? 1u : 0u); if (depth > c_maxstack) c_maxstack = depth; }   // entries incl. the nearest child, if its push fitted
                        if (S.sp < kStackMax) S.cur = rn;
                        else { need_pop = true; if (STATS) ++c_drops; }
                    }
                } else need_pop = true;
            
            }
            if (at_leaf) {
                // (a use of the fourth piece on this side as well: used by the node side alone its load would be moved into that side -- a second memory latency per step)
                asm volatile("" :: "v"(n3.x), "v"(n3.y), "v"(n3.z), "v"(n3.w));
                // a leaf whose triangle index is out of range points at the all-zero record behind the last triangle: the test
                // below fails on |det| < eps, as if it had not been made (renderer.wgsl:262); only the counter has to know
                if (STATS) { if ((S.cur & 0x7fffffffu) < 4u * A.num_tris) ++c_tris; }      // A.num_tris = the UBO's numTris <= uploaded
                // axis-major record (pt_host.h::TriRecord): piece a = (v0[a], e1[a], e2[a], n[a])
                const F3 v0 = f3(__uint_as_float(n0.x), __uint_as_float(n1.x), __uint_as_float(n2.x));
                const F3 e1 = f3(__uint_as_float(n0.y), __uint_as_float(n1.y), __uint_as_float(n2.y));
                const F3 e2 = f3(__uint_as_float(n0.z), __uint_as_float(n1.z), __uint_as_float(n2.z));
                // branch-free Moller-Trumbore (renderer.wgsl:185-205): same operations and comparisons,
                // rejections combined at the end, so the record is fetched in one go
                const F3 pv = cross3(S.d, e2);
                const float det = dot3(e1, pv);
                const bool ok_det = !(fabsf(det) < kTriEps);
                // 1 / det: the short correctly rounded form (pt_device.h::rcp_normal, 4 instructions fewer) in the kernel variant the host picks where it has
                // bounded |det| below that form's range for this scene and these cameras (a det below the range fails ok_det: its quotient is not used)
                const float inv_det = rcp_f<BOUNDED>(det);
                const F3 sv = S.o - v0;
                const float u = inv_det * dot3(sv, pv);
                const bool ok_u = !((u < 0.0f) | (u > 1.0f));
                const F3 q = cross3(sv, e1);
                const float v = inv_det * dot3(S.d, q);
                const bool ok_v = !((v < 0.0f) | ((u + v) > 1.0f));
                const float t = inv_det * dot3(e2, q);
                bool ok = ok_det & ok_u & ok_v & (t > kTriEps) & (t < S.best_t);
                // the UBO's numTris may be smaller than the uploaded triangle count: `ti < numTris` (renderer.wgsl:267) then hides the
                // triangles past it
                ok &= S.cur < A.tri_gate;          // (one unsigned compare: both sides carry the leaf bit; 0xFFFFFFFF, above every leaf reference, when nothing is hidden)
                if (ok) {
                    S.best_t = t; S.best_tri = S.cur;
                    if (S.bounce & kShadowBit) phase = kPhaseDone;   // any-hit: first accepted hit ends the ray
                }
                need_pop = true;
            }
            if (need_pop && phase == kPhaseTrav) {
                bool found = false;
                // deep entries (index >= kShort) live in the spill area: rare
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(S.sp > kShort) != 0ull, 0)) {     // wavefront-uniform: usually nobody is that deep
                    while (S.sp > kShort) {
                        --S.sp;
                        const unsigned long long e = *(volatile unsigned long long*)spill_at(S.sp - kShort);
                        if (__uint_as_float((uint32_t)(e >> 32)) < S.best_t) { S.cur = (uint32_t)e; found = true; break; }
                    }
                }
                if (!found && S.sp > 0) {
                    // Entries whose box the ray no longer reaches (tmin >= best) are skipped -- after a hit that is most of what a lane has
                    // stacked, and the wavefront loops as long as its slowest lane.  The loop is hand-written: per entry one address
                    // step, the read, two compares and three scalar instructions (lanes drop out of EXEC as they find their entry or run
                    // out of entries); the compiler's form of the same loop costs 5 vector + 10 scalar instructions per entry.
                    // (No manual wait states are needed inside: v_cmp -> s_and on VCC and s_and on EXEC -> the next vector instruction are
                    // interlocked on gfx9-family parts -- the compiler emits the same pairs back to back; EXEC is restored before the block
                    // ends, VCC is declared clobbered, LDS results are waited for with lgkmcnt(0).)
                    const uint32_t base = stk_lds, top = base + (uint32_t)S.sp * 512u;     // byte addresses: entry 0, one past the top entry
                    uint32_t addr = top, lo, hi; unsigned long long saved_exec;
                    asm volatile("s_mov_b64 %[save], exec\n"
                                 "1:\n\t"
                                 "v_add_u32 %[addr], 0xfffffe00, %[addr]\n\t"
                                 "ds_read_b32 %[hi], %[addr] offset:4\n\t"
                                 "ds_read_b32 %[lo], %[addr]\n\t"
                                 "s_waitcnt lgkmcnt(0)\n\t"
                                 "v_cmp_ngt_f32 vcc, %[best], %[hi]\n\t"         // not this one: go on
                                 "s_and_b64 exec, exec, vcc\n\t"
                                 "v_cmp_gt_u32 vcc, %[addr], %[base]\n\t"        // entries left below it
                                 "s_and_b64 exec, exec, vcc\n\t"
                                 "s_cbranch_execnz 1b\n\t"
                                 "s_mov_b64 exec, %[save]"
                                 : [addr] "+v"(addr), [lo] "=&v"(lo), [hi] "=&v"(hi), [save] "=&s"(saved_exec)
                                 : [best] "v"(S.best_t), [base] "v"(base)
                                 : "vcc", "memory");
                    found = __uint_as_float(hi) < S.best_t;          // the entry the lane stopped at: its own, or entry 0 when it ran out
                    S.sp = (int)((addr - base) >> 9);
                    if (found) S.cur = lo;
                }
                // a camera ray that found nothing leaves its sample at the primed miss value (0 + 1 * 0.01, renderer.wgsl:410): no shade pass, the lane is free
                if (!found) phase = ((S.bounce & kFlagsMask) == 0u && S.best_tri == kInvalidRef) ? kPhaseIdle : kPhaseDone;
            }
        }
        if (STATS) { const unsigned long long dt = __builtin_amdgcn_s_memtime() - cy_mark; cy_step += dt; if (!queue_empty) cy_step_q += dt; }
        // the conditions of the shade / refill passes, exactly as they are tested at the top of the outer loop, as ONE exit test (nothing traverses any more | a shade
        // pass is due | a refill is): tested one after the other they cost 26 scalar instructions per step on the way round the loop, like this 20
        const unsigned long long now_trav = __ballot(phase == kPhaseTrav);
        const unsigned long long now_done = __ballot(phase == kPhaseDone);
        trav_now = now_trav;
        const uint32_t n_done = (uint32_t)__popcll(now_done);
        // (a lane that neither traverses nor waits for a shade pass is idle -- no lane waits for a forked shadow ray where rays are still started: no third compare)
        const uint32_t n_idle = (uint32_t)__popcll(PT_LOOP_STAGE == 0 ? ~(now_trav | now_done) : __ballot(phase == kPhaseIdle));
        if ((int)(now_trav == 0ull) | (int)(n_done >= shade_due(now_trav | now_done)) | (int)(n_idle >= fill_thr)) break;
        }
#else
        // ------------------------------------------------------------------ the same steps with one ray per quad of lanes (see the top of pt_megakernel.hip)
        for (;;) {
        if (TIMELINE) { ++n_iter; lanes_sum += __popcll(trav_now); leaf_lanes += __popcll(trav_now & __ballot((S.cur & kLeaf) != 0u)); }      // wave-uniform: scalar counters
        if (STATS) { cy_mark = __builtin_amdgcn_s_memtime(); if (PT_LOOP_STAGE) { wait_seat_iters += __popcll(__ballot(phase == kPhaseWait)) >> (quad ? 2 : 0); live_seat_iters += __popcll(__ballot(phase != kPhaseIdle && !(S.bounce & kForkedBit))) >> (quad ? 2 : 0); } }
        if (lane_of(trav_now)) {
            bool need_pop = false;
            if (STATS) { ++path_steps; ++ray_steps; if (S.bounce & kShadowBit) ++path_shadow_steps; }
            const bool at_leaf = (S.cur & kLeaf) != 0u;
            // this lane's 16-byte piece of the record its ray stands at: child qk of a node, axis qk of a triangle (lane 3 of a quad at a
            // leaf reads the record's normal: not used here).  One load before the node / leaf branch.
            uint4 n = *(const uint4*)((const char*)A.scene + ((S.cur << 4) + (qk << 4)));
            asm volatile("" : "+v"(n.x), "+v"(n.y), "+v"(n.z), "+v"(n.w));
            if (at_leaf) {
                if (STATS) { if (qk == 0u && (S.cur & 0x7fffffffu) < 4u * A.num_tris) ++c_tris; }
                // Moller-Trumbore (renderer.wgsl:185-205) with axis c = qk in lane c of the quad: cross3(a, b)[c] = a[c+1] b[c+2] - a[c+2] b[c+1]
                // (indices mod 3), dot3 = (x + y) + z by broadcasts -- operation for operation the one-lane form above
                const float v0c = __uint_as_float(n.x), e1c = __uint_as_float(n.y), e2c = __uint_as_float(n.z);
                const bool k1 = qk == 1u, k2 = qk == 2u;
                const float oc = k2 ? S.o.z : (k1 ? S.o.y : S.o.x), dc = k2 ? S.d.z : (k1 ? S.d.y : S.d.x);
                const float d1 = k2 ? S.d.x : (k1 ? S.d.z : S.d.y), d2 = k2 ? S.d.y : (k1 ? S.d.x : S.d.z);       // d[c+1], d[c+2]
                const float pvc = d1 * dpp_f<kQuadRot2>(e2c) - d2 * dpp_f<kQuadRot1>(e2c);                              // cross3(d, e2)[c]
                const float det = quad_dot3(e1c * pvc);
                const bool ok_det = !(fabsf(det) < kTriEps);
                const float inv_det = rcp_f<BOUNDED>(det);
                const float svc = oc - v0c;
                const float u = inv_det * quad_dot3(svc * pvc);
                const bool ok_u = !((u < 0.0f) | (u > 1.0f));
                const float qc = dpp_f<kQuadRot1>(svc) * dpp_f<kQuadRot2>(e1c) - dpp_f<kQuadRot2>(svc) * dpp_f<kQuadRot1>(e1c);   // cross3(sv, e1)[c]
                const float v = inv_det * quad_dot3(dc * qc);
                const bool ok_v = !((v < 0.0f) | ((u + v) > 1.0f));
                const float t = inv_det * quad_dot3(e2c * qc);
                bool ok = ok_det & ok_u & ok_v & (t > kTriEps) & (t < S.best_t);
                ok &= S.cur < A.tri_gate;          // (one unsigned compare: both sides carry the leaf bit; 0xFFFFFFFF, above every leaf reference, when nothing is hidden)
                if (ok) {
                    S.best_t = t; S.best_tri = S.cur;
                    if (S.bounce & kShadowBit) phase = kPhaseDone;   // any-hit: first accepted hit ends the ray
                }
                need_pop = true;
            } else {
                float tk;
                const unsigned long long H = slab_sel(S.o, S.inv, S.sel, n.x, n.y, n.z, S.best_t, tk);      // this lane's child box
                if (STATS) c_nodes += (n.w != kInvalidRef) ? 1u : 0u;                                        // every lane counts its own child slot
                const uint32_t hn = quad_nibble(H, lane);                                                     // the ray's hit children
                if (hn != 0u) {
                    // renderer.wgsl:314-342 for one ray, a child per lane: hit children keep slot order; the first minimum of tmin is entered
                    // next and trades places with the first hit; the others are stacked far -> near, i.e. the child at place j of the
                    // hit list (after the swap) goes to sp + (hits - 1 - j).  Each stacked child is written by its own lane.
                    const bool h = lane_of(H);
                    const float e = h ? tk : 3.0e38f;
                    const float tn = quad_min_f32(e);
                    const uint32_t en = quad_nibble(__builtin_amdgcn_ballot_w64(e == tn), lane);           // slots at the minimum (hit slots: tn < 3e38)
                    const uint32_t near_slot = (uint32_t)__builtin_ctz(en);
                    const uint32_t hits = (uint32_t)__popc(hn);
                    const uint32_t j_own = (uint32_t)__popc(hn & q_low), j_near = (uint32_t)__popc(hn & ((1u << near_slot) - 1u));
                    const bool is_near = qk == near_slot;
                    const uint32_t j = (j_own == 0u) ? j_near : j_own;               // the first hit takes the place the nearest child left
                    const int pos = S.sp + (int)(hits - 1u - j);
                    if (h && !is_near) {
                        const unsigned long long w = ((unsigned long long)__float_as_uint(tk) << 32) | n.w;
                        if (__builtin_expect(pos < kShort, 1)) *qstk_at(pos) = w;
                        else if (pos < kStackMax) { *qspill_at(pos - kShort) = w; if (STATS) ++spill_ops; }
                        else if (STATS) ++c_drops;                                   // beyond the 64 entries: dropped (renderer.wgsl:337)
                        if (STATS) { ++push_ops; if (pos >= 8) ++push8_ops; if (pos >= 12) ++push12_ops; }
                    }
                    const uint32_t rn = quad_or(is_near ? n.w : 0u);
                    const int sp_all = S.sp + (int)hits - 1;                        // entries below the nearest child once everything is pushed
                    S.sp = sp_all < kStackMax ? sp_all : kStackMax;
                    if (STATS) { const uint32_t depth = (uint32_t)S.sp + (sp_all < kStackMax ? 1u : 0u); if (depth > c_maxstack) c_maxstack = depth; }
                    if (sp_all < kStackMax) S.cur = rn;                              // the push of the nearest child would have fitted
                    else { need_pop = true; if (STATS && is_near) ++c_drops; }
                } else need_pop = true;
            }
            if (need_pop && phase == kPhaseTrav) {
                bool found = false;
                if (__builtin_expect(__builtin_amdgcn_ballot_w64(S.sp > kShort) != 0ull, 0)) {     // deep entries live in the spill area: rare, one at a time
                    while (S.sp > kShort) {
                        --S.sp;
                        const unsigned long long e = *(volatile unsigned long long*)qspill_at(S.sp - kShort);
                        if (__uint_as_float((uint32_t)(e >> 32)) < S.best_t) { S.cur = (uint32_t)e; found = true; break; }
                    }
                }
                // four entries per round: lane k looks at entry sp-1-k; the first of them (from the top) that the ray still reaches is the next node
                while (!found && S.sp > 0) {
                    const int idx = S.sp - 1 - (int)qk;
                    unsigned long long e = 0ull;
                    if (idx >= 0) e = *qstk_at(idx);
                    const bool reach = idx >= 0 && __uint_as_float((uint32_t)(e >> 32)) < S.best_t;
                    const uint32_t rm = quad_nibble(__builtin_amdgcn_ballot_w64(reach), lane);
                    if (rm != 0u) {
                        const uint32_t kf = (uint32_t)__builtin_ctz(rm);
                        S.cur = quad_or(qk == kf ? (uint32_t)e : 0u);
                        S.sp = S.sp - 1 - (int)kf;
                        found = true;
                    } else S.sp = S.sp > 4 ? S.sp - 4 : 0;
                }
                if (!found) phase = ((S.bounce & kFlagsMask) == 0u && S.best_tri == kInvalidRef) ? kPhaseIdle : kPhaseDone;
            }
        }
        if (STATS) { const unsigned long long dt = __builtin_amdgcn_s_memtime() - cy_mark; cy_step += dt; if (!queue_empty) cy_step_q += dt; }
        const unsigned long long now_trav = __ballot(phase == kPhaseTrav);
        const unsigned long long now_done = __ballot(phase == kPhaseDone);
        trav_now = now_trav;
        // one exit test, as in the loop above (a dry source -- every wavefront that re-seated its paths -- never compares the idle lanes)
        if ((int)(now_trav == 0ull) | (int)((uint32_t)__popcll(now_done) >= shade_due(now_trav | now_done)) | (int)(fill_thr < 0x10000u && (uint32_t)__popcll(__ballot(phase == kPhaseIdle)) >= fill_thr)) break;
        }
#endif
    }
