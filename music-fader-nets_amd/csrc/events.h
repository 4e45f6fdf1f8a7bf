// events.h - the reading of a row of event tokens that attributes.hip, notes.hip and constrain.hip share: token ranges, the clocked events of a row
// in LDS, and the walk that pairs note-ons with what closes them.  include/fadernets.h has the definition (tokens -> timed notes).
#pragma once
#include "common.h"

// offset of token e in the range of n tokens that starts at lo, or -1 (64-bit difference: lo is whatever the memory held)
__device__ __forceinline__ int fn_token_offset(int e, int lo, int n) {
    const long d = (long)e - (long)lo;
    return (d >= 0 && d < n) ? (int)d : -1;
}

// Phase 1 of a one-wavefront-per-row kernel: the row's end (a ballot for the eos), the clock of every token (a scan of the shift amounts) and the
// events into LDS: ev[i] = tick << 9 | code for i < len (code 0 = skipped, 1 + p = note-on, 129 + p = note-off; the tick is the clock AFTER the token).
// VEL: also vel[i], the velocity current at token i (a carry-forward scan from c.def_vel on).  c: a view with on_lo, off_lo, np, shift_lo, ns, eos,
// vocab - and vel_lo, nv, vstep, def_vel where VEL.  Returns len <= steps; t_end is the clock at the row's end.  All 64 lanes call it together; the
// caller's barrier stands between these stores and their readers.
template <bool VEL, class View>
__device__ __forceinline__ int fn_event_scan(const int32_t* __restrict__ row, int steps, int lane, const View& c, uint32_t* ev, uint8_t* vel, uint32_t& t_end) {
    int len = steps;
    uint32_t carry = 0, vcarry = 0;
    if constexpr (VEL) vcarry = (uint32_t)c.def_vel;
    bool found = false;
    for (int base = 0; base < steps && !found; base += 64) {
        const int i = base + lane;
        const int e = i < steps ? row[i] : 0;
        const unsigned long long m = __ballot(i < steps && c.eos >= 0 && e == c.eos);
        if (m != 0ull) found = true, len = base + __ffsll((long long)m) - 1;
        const bool live = i < len;                      // len <= steps
        uint32_t amount = 0, code = 0, v = 0;
        if (live && (c.vocab <= 0 || (e >= 0 && e < c.vocab))) {
            int p;
            if ((p = fn_token_offset(e, c.on_lo, c.np)) >= 0) code = 1u + (uint32_t)p;
            else if ((p = fn_token_offset(e, c.off_lo, c.np)) >= 0) code = 129u + (uint32_t)p;
            else if ((p = fn_token_offset(e, c.shift_lo, c.ns)) >= 0) amount = (uint32_t)p + 1u;
            else if constexpr (VEL) {
                if ((p = fn_token_offset(e, c.vel_lo, c.nv)) >= 0) v = (uint32_t)min(1 + p * c.vstep, 127);
            }
        }
        const uint32_t x = fn_wave_scan_add(amount, lane);
        if constexpr (VEL) {
            v = fn_wave_scan_last(v, lane);
            if (v == 0u) v = vcarry;
        }
        if (live) {
            ev[i] = ((carry + x) << 9) | code;
            if constexpr (VEL) vel[i] = (uint8_t)v;
        }
        carry += __shfl(x, 63, 64);
        if constexpr (VEL) vcarry = __shfl(v, 63, 64);
    }
    t_end = carry;
    return len;
}

// One walk over the row's stored events by every lane (the same LDS word for all: a broadcast); lane l follows pitches l and l + 64 and keeps their
// open t0, and the index of the note-on token that opened them, in registers.  closed(pitch, t0, t1, at) is called for every kept note (t1 > t0) of
// the lane's two pitches as it closes: by a later event of its pitch, or at t_end.
template <class F>
__device__ __forceinline__ void fn_note_walk(const uint32_t* ev, int len, uint32_t t_end, int lane, F&& closed) {
    int open0 = -1, open1 = -1, at0 = 0, at1 = 0;
    for (int i = 0; i < len; ++i) {
        const uint32_t w = ev[i];
        const int code = (int)(w & 511u);
        if (code == 0) continue;
        const bool is_on = code <= 128;
        const int p = is_on ? code - 1 : code - 129;
        if ((p & 63) != lane) continue;
        const uint32_t t = w >> 9;
        const int open = (p >> 6) ? open1 : open0, at = (p >> 6) ? at1 : at0;
        if (open >= 0 && t > (uint32_t)open) closed(p, (uint32_t)open, t, at);
        const int now = is_on ? (int)t : -1;
        if (p >> 6) open1 = now, at1 = i; else open0 = now, at0 = i;
    }
    if (open0 >= 0 && t_end > (uint32_t)open0) closed(lane, (uint32_t)open0, t_end, at0);
    if (open1 >= 0 && t_end > (uint32_t)open1) closed(lane + 64, (uint32_t)open1, t_end, at1);
}
