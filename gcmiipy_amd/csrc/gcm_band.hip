// gcm_band_run: the library-driven band loop and the ghost-row exchange it posts itself (gcm_set_exchange).  Host
// code only; stepping and the ghost rows' pack / unpack are gcmcore.hip's and the phases behind a GCM_PE25D step are
// gcm_pe.hip's, reached through gcm_handle.h and the C ABI.
#include <cstdlib>

#include "gcm_handle.h"

using namespace gcm;

extern "C" {

int gcm_set_exchange(gcm_handle *h, const gcm_exchange *x) {
    if (int rc = band_only(h, "gcm_set_exchange")) return rc;
    GcmBandExchange &b = h->band;
    if (!x) {
        b.set = false;
        if (h->pe) return pe25d_set_halo_buffers(h->pe, nullptr, nullptr, h->stream, &h->err);
        return GCM_OK;
    }
    const int nfn = (x->send != nullptr) + (x->recv != nullptr) + (x->group_start != nullptr) + (x->group_end != nullptr);
    if (nfn != 0 && nfn != 4) return fail(h, GCM_ERR_ARG, "gcm_set_exchange: give all four RCCL entry points, or none (loopback)");
    if (nfn == 4 && !x->comm) return fail(h, GCM_ERR_ARG, "gcm_set_exchange: communicator is NULL");
    if (!x->send_north || !x->send_south || !x->recv_north || !x->recv_south)
        return fail(h, GCM_ERR_ARG, "gcm_set_exchange: four device buffers of gcm_halo_bytes() are required");
    if (int rc = select_device(h)) return rc;
    void *cs = nullptr;
    if (int rc = gcm_comm_stream(h, &cs)) return rc;
    if (!b.ev_pack) HIPCHK(h, hipEventCreateWithFlags(&b.ev_pack, hipEventDisableTiming));
    if (!b.ev_comm) HIPCHK(h, hipEventCreateWithFlags(&b.ev_comm, hipEventDisableTiming));
    b.xch = *x;
    b.set = true;
    b.primed = false;
    if (const char *e = getenv("GCM_BAND_OVERLAP")) b.overlap = e[0] == '1';
    if (h->pe) pe25d_set_edges_first(h->pe, b.overlap);
    const char *oc = getenv("GCM_BAND_COMM_STREAM");        // diagnostic: the exchange on the comm stream, a join per stage (round 1)
    b.on_comm = oc && oc[0] == '1';
    // GCM_PE25D: the edge rows of a stage are updated and packed into the send buffers on the handle's second stream (gcm_set_halo_buffers)
    if (h->pe) return pe25d_set_halo_buffers(h->pe, x->send_north, x->send_south, h->stream, &h->err);
    return GCM_OK;
}

int gcm_set_band_overlap(gcm_handle *h, int on) {
    if (int rc = band_only(h, "gcm_set_band_overlap")) return rc;
    h->band.overlap = on != 0;
    if (h->pe) pe25d_set_edges_first(h->pe, h->band.overlap);
    return GCM_OK;
}

}  // extern "C"

// pack both edges on the compute stream; the comm stream waits for the pack only
static int pack_edges(gcm_handle *h) {
    if (int rc = gcm_halo_pack2(h, h->band.xch.send_north, h->band.xch.send_south, h->stream)) return rc;
    HIPCHK(h, hipEventRecord(h->band.ev_pack, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm, h->band.ev_pack, 0));
    return GCM_OK;
}

// the send buffers are packed (or being packed: the caller has made cs wait for that); post the ring exchange
// on cs.  On the comm stream (a stream of its own, never the compute or the second stream) ev_comm follows it ...
static int band_post(gcm_handle *h, hipStream_t cs) {
    const gcm_exchange &x = h->band.xch;
    const size_t nbytes = gcm_halo_bytes(h);
    if (x.send) {
        int rc = x.group_start();
        if (rc == 0) {
            // north edge first, then the south ghost first: with two ranks both neighbours are the same peer and the i-th send
            // must meet the peer's i-th receive
            int r1 = x.send(x.send_north, nbytes, 0 /*ncclChar*/, x.north, x.comm, cs);
            int r2 = r1 ? r1 : x.send(x.send_south, nbytes, 0, x.south, x.comm, cs);
            int r3 = r2 ? r2 : x.recv(x.recv_south, nbytes, 0, x.south, x.comm, cs);
            int r4 = r3 ? r3 : x.recv(x.recv_north, nbytes, 0, x.north, x.comm, cs);
            const int re = x.group_end();                   // always closed, whatever a call returned
            rc = r4 ? r4 : re;
        }
        if (rc != 0) {
            char b[96];
            snprintf(b, sizeof b, "gcm_band_run: RCCL call failed (ncclResult %d)", rc);
            return fail(h, GCM_ERR_HIP, b);
        }
    } else {
        // loopback: what goes north arrives as this band's own south ghost rows and vice versa
        // (GCM_BAND_EXCHANGE_DELAY_US: a stand-in for the transfer time between two devices, which one GPU cannot
        // show -- tools/tools_band_time.py sweeps it to see how much exchange latency an orchestration hides)
        static const double delay_us = getenv("GCM_BAND_EXCHANGE_DELAY_US") ? atof(getenv("GCM_BAND_EXCHANGE_DELAY_US")) : 0.0;
        launch_spin(cs, delay_us);
        HIPCHK(h, hipMemcpyAsync(x.recv_south, x.send_north, nbytes, hipMemcpyDeviceToDevice, cs));
        HIPCHK(h, hipMemcpyAsync(x.recv_north, x.send_south, nbytes, hipMemcpyDeviceToDevice, cs));
    }
    if (cs == h->comm) HIPCHK(h, hipEventRecord(h->band.ev_comm, cs));
    return GCM_OK;
}
// ... and the other half: the compute stream waits for the exchange and fills the ghost rows
static int band_finish(gcm_handle *h) {
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->band.ev_comm, 0));
    return gcm_halo_unpack2(h, h->band.xch.recv_north, h->band.xch.recv_south, h->stream);
}
static int band_exchange(gcm_handle *h) {
    const int rc = band_post(h, h->comm);
    return rc ? rc : band_finish(h);
}

// one GCM_PE25D band step: per Euler stage the edge rows + pack on the library's second stream, the interior
// rows on the compute stream, then the exchange and the unpack behind the pack on that same second stream
// (they overlap the interior rows).  The compute stream carries K2a -> K3 -> K4 of the band's OWN rows and
// never reads a ghost row (pe25d_kernels.hip, half_t), so it does not wait for the exchange: everything that
// reads ghost rows -- the next stage's K1, column sums, edge rows -- is queued on the second stream, behind
// the unpack, in stream order.  gcm_band_run joins the two streams once, when it returns.
// GCM_BAND_COMM_STREAM=1: the exchange on the comm stream and a join per stage, as in round 1.
// The phases registered behind the dynamics (solar step, Held-Suarez ... the climatology's sample) are gcm_pe.hip's: the
// ghost rows' on the second stream right behind the corrector's unpack and ahead of the ghost rows' column sums and
// anchors (pe_ghost_row_phases), the own rows' at the end of the step on the compute stream (pe_own_row_phases), which
// takes the ghost rows with it when the exchange was joined into the compute stream.
// With the boundary layer registered (the band has opted in: gcm_set_band_boundary_layer) the walk splits at it and the
// step takes a THIRD exchange, of the current state's edge rows as the boundary layer left them (band_step_pe_bl).
// With the horizontal diffusion registered (the band has opted in: gcm_set_band_hdiff) the own rows are diffused right
// behind the corrector's unpack and the current state's edge rows are exchanged once more AHEAD of the walk
// (band_step_pe_hd); the ghost rows' phases and their column sums then follow that exchange's unpack, not the
// corrector's.  With both registered a step takes four exchanges.
// Without either band_step_pe queues what it always has: no event, launch or copy more.
static int band_step_pe_bl(gcm_handle *h, double dt, hipStream_t ax);
static int band_step_pe_hd(gcm_handle *h, double dt, hipStream_t ax, bool bl);
static int band_step_pe(gcm_handle *h, double dt) {
    int rc = GCM_OK;
    hipStream_t ax = h->band.on_comm ? nullptr : pe25d_aux_stream(h->pe);
    const bool bl = band_boundary_layer_on(h), hd = band_hdiff_on(h);
    for (int stage = 0; stage < 2; ++stage) {
        if ((rc = pe25d_step_phase(h->pe, 2 * stage, dt, h->stream, &h->err, ax != nullptr))) return rc;
        if (ax) {
            if ((rc = band_post(h, ax))) return rc;
            if ((rc = gcm_halo_unpack2(h, h->band.xch.recv_north, h->band.xch.recv_south, ax))) return rc;
            // (the corrector's ghost rows of a band with the diffusion: read by the own rows' launch, then overwritten by the
            // exchange behind it, whose unpack the ghost rows' phases follow: band_step_pe_hd)
            if (stage == 1 && !hd && (rc = pe_ghost_row_phases(h, dt, ax, bl ? kPhasesHead : kPhasesAll))) return rc;
            // (the corrector's ghost rows of a band with the boundary layer: overwritten by the third exchange, behind
            // which their column sums and anchors are queued; until then nothing on `ax` reads own rows' u and v)
            if (!((bl || hd) && stage == 1) && (rc = pe25d_prep_ghost_rows(h->pe, &h->err))) return rc;
            h->band.join_pending = true;
        }
        if ((rc = pe25d_step_phase(h->pe, 2 * stage + 1, dt, h->stream, &h->err, ax != nullptr))) return rc;
        if (!ax) {
            if ((rc = pe25d_wait_edges(h->pe, h->comm, &h->err))) return rc;
            if ((rc = band_exchange(h))) return rc;
        }
    }
    if (hd && (rc = band_step_pe_hd(h, dt, ax, bl))) return rc;
    if (bl) return band_step_pe_bl(h, dt, ax);
    return pe_own_row_phases(h, dt, phase_ghosts(h, ax != nullptr), ax != nullptr, ax, kPhasesAll);
}

// The horizontal diffusion of a band step, behind the corrector (the swap is done: the current state is the new one, and
// packs and unpacks take it) and ahead of the phase walk.
//   compute stream: [ax: -> ev_comm @ ax, waits: the corrector's unpack, and every read of the send buffers by the
//                   corrector's exchange],
//                   the diffusion of the own rows, which reads ghost rows -2, -1, H, H + 1 of the selected fields; the copy
//                   back; the pack of the edge rows as it left them -> ev_pack
//   ax / comm:      waits ev_pack; the exchange, in the existing message and buffers (the tracers' edge rows ride in it as
//                   in the boundary layer's third exchange); (ax:) the unpack, the ghost rows' solar step + Held-Suarez
//                   (without the boundary layer: + convective adjustment + moist physics, their column sums and anchors)
//   compute stream: (comm: waits ev_comm, the unpack;) the walk as it was, beside the exchange on `ax`
// The corrector's unpack is behind the compute stream in the comm orchestration already (band_exchange).  The new unpack
// follows ev_pack, hence every read of the ghost rows by the diffusion.  The events are the run's own (ev_comm, ev_pack),
// each waited for in stream order before it is recorded again.
// Not built: the edge rows' tiles first, with the exchange beside the interior tiles.  The launch is out of place and
// the interior tiles read the original edge rows, so these cannot be copied back and packed while it is in flight.
static int band_step_pe_hd(gcm_handle *h, double dt, hipStream_t ax, bool bl) {
    int rc = GCM_OK;
    if (ax) {
        HIPCHK(h, hipEventRecord(h->band.ev_comm, ax));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->band.ev_comm, 0));
    }
    if ((rc = pe_band_hdiff_rows(h, ax != nullptr))) return rc;
    if (!ax) {                                             // (pack -> ev_pack @ st, comm waits; the group; st waits, the unpack)
        if ((rc = pack_edges(h)) || (rc = band_exchange(h))) return rc;
        return GCM_OK;
    }
    if ((rc = gcm_halo_pack2(h, h->band.xch.send_north, h->band.xch.send_south, h->stream))) return rc;
    HIPCHK(h, hipEventRecord(h->band.ev_pack, h->stream));
    HIPCHK(h, hipStreamWaitEvent(ax, h->band.ev_pack, 0));
    if ((rc = band_post(h, ax))) return rc;
    if ((rc = gcm_halo_unpack2(h, h->band.xch.recv_north, h->band.xch.recv_south, ax))) return rc;
    if ((rc = pe_ghost_row_phases(h, dt, ax, bl ? kPhasesHead : kPhasesAll))) return rc;
    if (!bl && (rc = pe25d_prep_ghost_rows(h->pe, &h->err))) return rc;
    return GCM_OK;
}

// The end of a band step with the boundary layer registered, behind the corrector (the swap is done: the current state
// is the new one, and packs and unpacks take it -- no phase pending, pack_set < 0, no star).
//   compute stream: solar step + Held-Suarez of the own rows (with the exchange on the comm stream: of the ghost rows too),
//                   [ax: -> ev_comm @ ax, waits: the corrector's unpack and the ghost rows' solar step + Held-Suarez],
//                   the boundary layer over the own rows, which reads v of ghost row -1 and all of ghost row H,
//                   the pack of the edge rows as it left them -> ev_pack
//   ax / comm:      waits ev_pack; the exchange; (ax:) the unpack, the ghost rows' convective adjustment + moist physics,
//                   their column sums and anchors (pe25d_prep_ghost_rows)
//   compute stream: (comm: waits ev_comm, the unpack;) convective adjustment + moist physics of the own rows (comm: and of
//                   the ghost rows), beside the exchange on `ax`; the sample joins the tail of `ax` first
// The wait for `ax` also frees the send buffers (the corrector's exchange has read them) and keeps the third unpack,
// which follows ev_pack, behind every read of the ghost rows by the boundary layer.  The events are the run's own
// (ev_comm, ev_pack), each waited for in stream order before it is recorded again.
static int band_step_pe_bl(gcm_handle *h, double dt, hipStream_t ax) {
    int rc = GCM_OK;
    // (the head's walk makes the compute stream wait for `ax` ahead of the boundary layer: -> ev_comm @ ax)
    if ((rc = pe_own_row_phases(h, dt, phase_ghosts(h, ax != nullptr), ax != nullptr, ax, kPhasesHead))) return rc;
    if (!ax) {                                             // (pack -> ev_pack @ st, comm waits; the group; st waits, the unpack)
        if ((rc = pack_edges(h)) || (rc = band_exchange(h))) return rc;
    } else {
        if ((rc = gcm_halo_pack2(h, h->band.xch.send_north, h->band.xch.send_south, h->stream))) return rc;
        HIPCHK(h, hipEventRecord(h->band.ev_pack, h->stream));
        HIPCHK(h, hipStreamWaitEvent(ax, h->band.ev_pack, 0));
        if ((rc = band_post(h, ax))) return rc;
        if ((rc = gcm_halo_unpack2(h, h->band.xch.recv_north, h->band.xch.recv_south, ax))) return rc;
        if ((rc = pe_ghost_row_phases(h, dt, ax, kPhasesTail))) return rc;
        if ((rc = pe25d_prep_ghost_rows(h->pe, &h->err))) return rc;
    }
    return pe_own_row_phases(h, dt, phase_ghosts(h, ax != nullptr), ax != nullptr, ax, kPhasesTail);
}

static int run_pe(gcm_handle *h, int nsteps, double dt) {
    int rc = pe_phase_tables(h, nsteps, dt);
    if (rc) return rc;
    if (!h->band.primed) {                                 // ghost rows of the initial state (and of the ground temperature), once
        if ((rc = pack_edges(h)) || (rc = band_exchange(h))) return rc;
        h->band.primed = true;
    }
    for (int n = 0; n < nsteps; ++n)
        if ((rc = band_step_pe(h, dt))) return rc;
    if (h->band.join_pending) {
        // the one join of the run: what follows on the compute stream (the caller's gcm_get_state, diagnostics, the next run)
        // also follows the last unpack on the second stream
        hipStream_t ax = pe25d_aux_stream(h->pe);
        HIPCHK(h, hipEventRecord(h->band.ev_comm, ax));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->band.ev_comm, 0));
        h->band.join_pending = false;
    }
    pe25d_join_third_stream(h->pe, h->stream);
    pe25d_join_tracers(h->pe, h->stream);                 // (a band's tracers: the last stage's launches)
    return GCM_OK;
}

// one exchange per step, overlapped with the rows that need no ghost data
static int run_exchange_per_step(gcm_handle *h, int nsteps, double dt) {
    int rc = GCM_OK;
    for (int n = 0; n < nsteps; ++n) {
        if ((rc = pack_edges(h))) return rc;
        if ((rc = gcm_step_interior(h, dt, h->stream))) return rc;
        if ((rc = band_exchange(h))) return rc;
        if ((rc = gcm_step_boundary(h, dt, h->stream))) return rc;
    }
    return GCM_OK;
}

// deep halo, an exchange every k steps with nothing beside it
static int run_deep(gcm_handle *h, int nsteps, double dt) {
    const int k = h->G / kGhost;
    int rc = GCM_OK;
    for (int done = 0; done < nsteps;) {
        if (!h->band.primed || h->since_exchange >= k) {
            // nothing runs beside this exchange, so it goes on the compute stream itself: pack, send/recv group, unpack in stream
            // order (on a second stream the two cross-queue dependencies cost 11 us each -- trace of the N = 8 band -- a quarter of the exchange)
            if ((rc = gcm_halo_pack2(h, h->band.xch.send_north, h->band.xch.send_south, h->stream))) return rc;
            if ((rc = band_post(h, h->stream))) return rc;
            if ((rc = gcm_halo_unpack2(h, h->band.xch.recv_north, h->band.xch.recv_south, h->stream))) return rc;
            h->band.primed = true;
        }
        const int n = std::min(k - h->since_exchange, nsteps - done);
        if ((rc = gcm_step(h, n, dt))) return rc;
        done += n;
    }
    return GCM_OK;
}

// Deep halo (an exchange every k steps) with the exchange hidden behind two steps' interior rows.  The LAST step of a window
// produces the G edge rows of either side first; they are packed and sent while the rest of that step runs.  The FIRST step of
// the next window starts with the rows that need no ghost data; only then does the compute stream wait for the exchange, fill
// the ghost rows and produce the rows next to them.  Same kernels on the same rows as the plain sequence: bit-identical.
static int window_first(gcm_handle *h, double dt) {         // split around the unpack
    const int H = h->H, e = h->G - kGhost;
    step_rows(h, dt, kGhost, H - kGhost, h->stream);
    if (int rc = band_finish(h)) return rc;                 // (resets since_exchange)
    h->band.inflight = false;
    step_rows(h, dt, -e, kGhost, h->stream);
    step_rows(h, dt, H - kGhost, H + e, h->stream);
    swap_state(h);
    h->since_exchange = 1;
    return GCM_OK;
}
static void window_middle(gcm_handle *h, double dt) {       // as gcm_step: the valid ghost rows shrink by kGhost a step
    const int e = h->G - kGhost * (h->since_exchange + 1);
    step_rows(h, dt, -e, h->H + e, h->stream);
    swap_state(h);
    ++h->since_exchange;
}
static int window_last(gcm_handle *h, double dt) {          // edges first: no ghost rows left to use
    const int H = h->H, G = h->G;
    step_rows(h, dt, 0, G, h->stream);
    step_rows(h, dt, H - G, H, h->stream);
    swap_state(h);                                          // the pack reads the state being produced
    int rc = pack_edges(h);
    swap_state(h);
    if (rc || (rc = band_post(h, h->comm))) return rc;
    h->band.inflight = true;
    step_rows(h, dt, G, H - G, h->stream);
    swap_state(h);
    h->since_exchange = h->G / kGhost;
    return GCM_OK;
}
static int run_deep_overlapped(gcm_handle *h, int nsteps, double dt) {
    GcmBandExchange &b = h->band;
    const int k = h->G / kGhost;
    int rc = GCM_OK, done = 0;
    while (done < nsteps) {
        if (!b.primed || (h->since_exchange >= k && !b.inflight)) {
            if ((rc = pack_edges(h)) || (rc = band_post(h, h->comm))) return rc;
            b.inflight = b.primed = true;
        }
        if (b.inflight) {
            if ((rc = window_first(h, dt))) return rc;
            ++done;
        }
        for (; done < nsteps && h->since_exchange < k - 1; ++done) window_middle(h, dt);
        if (done < nsteps && h->since_exchange == k - 1) {
            if ((rc = window_last(h, dt))) return rc;
            ++done;
        }
    }
    if (b.inflight) {                                       // nothing is left pending across calls
        if ((rc = band_finish(h))) return rc;
        b.inflight = false;
    }
    return GCM_OK;
}

// What gcm_band_run queues, by orchestration (st = the handle's stream, comm = gcm_comm_stream, ax = GCM_PE25D's second stream;
// "-> E @ s": event E recorded on s behind what the line names; "s waits E": hipStreamWaitEvent):
//   orchestration          pack              send/recv  unpack  events
//   run_pe, first exchange st                comm       st      pack -> ev_pack @ st, comm waits; group -> ev_comm @ comm, st waits
//   run_pe, every stage    ax (pe25d: with   ax         ax      none per stage: stream order on ax.  When the run returns:
//                          the edge rows)                       -> ev_comm @ ax, st waits
//                                                               a step that ends with a climatology or spectra sample: -> ev_comm @ ax, st waits ahead of the sample
//   .. boundary layer on   st (third exch.:  ax         ax      behind the corrector's unpack and the ghost rows' solar + Held-Suarez: -> ev_comm @ ax, st waits
//      (third exchange)    the current                          ahead of the own rows' boundary layer; pack -> ev_pack @ st, ax waits; the ghost rows'
//                          state's edge rows)                   convect + moist and their column sums follow the unpack on ax
//   .. diffusion on        st (behind the    ax         ax      behind the corrector's unpack: -> ev_comm @ ax, st waits ahead of the own rows' diffusion and its
//      (one more exchange) copy back: the                       copy back; pack -> ev_pack @ st, ax waits; the ghost rows' phases and their column sums follow the
//                          current state's edge rows)           new unpack on ax (with the boundary layer on: its head only, the rest as in the lines above)
//   .. GCM_BAND_COMM_STREAM=1  ax (as above) comm       st      comm waits for the edge rows' pack (pe25d_wait_edges); group -> ev_comm @ comm, st waits
//      .. boundary layer on  st (third exch.) comm      st      pack -> ev_pack @ st, comm waits; group -> ev_comm @ comm, st waits ahead of the unpack
//      .. diffusion on     st (one more)     comm       st      behind the corrector's unpack on st: the diffusion, the copy back; pack -> ev_pack @ st, comm waits;
//                                                               group -> ev_comm @ comm, st waits ahead of the unpack and the walk
//   run_exchange_per_step  st                comm       st      pack -> ev_pack @ st, comm waits; group -> ev_comm @ comm, st waits ahead of the boundary rows
//   run_deep               st                st         st      none: stream order
//   run_deep_overlapped    st (window_last,  comm       st      pack -> ev_pack @ st, comm waits; group -> ev_comm @ comm; st waits in window_first behind
//                          or a new state)                      its interior rows, or when the run returns
extern "C" int gcm_band_run(gcm_handle *h, int nsteps, double dt) {
    if (!h || nsteps < 0) return GCM_ERR_ARG;
    if (int rc = band_only(h, "gcm_band_run")) return rc;
    if (!h->band.set) return fail(h, GCM_ERR_STATE, "gcm_band_run: no exchange registered (gcm_set_exchange)");
    if (int rc = select_device(h)) return rc;
    if (h->pe) return run_pe(h, nsteps, dt);
    const int k = h->G / kGhost;                            // steps per exchange
    const bool overlap = k > 1 && h->band.overlap && h->H > 2 * h->G + 2 * kGhost;
    if (int rc = k == 1 ? run_exchange_per_step(h, nsteps, dt)
                 : overlap ? run_deep_overlapped(h, nsteps, dt) : run_deep(h, nsteps, dt))
        return rc;
    h->star_valid = false;
    return launch_status(h);
}
