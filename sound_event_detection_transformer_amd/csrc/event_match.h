// event_match.h - sed_eval's event-based matching of one clip, shared by event_metrics_kernel (metrics.hip: estimates = the queries
// it just decoded) and event_sweep_kernel (sweep.hip: estimates = the slots of an event record).  One wave; the arrays are the
// caller's LDS.  Estimates are numbered 0 .. 63 (one lane each when the hit graph is built), reference events 0 .. ne - 1 in table order.
//   * event_hit_graph     adj[j] bit q = estimate q hits reference j
//   * event_class_match   tp of one class: maximum-cardinality matching (augmenting paths, breadth first) or sed_eval's greedy pass
// The classes of a clip are matched by different lanes at once: they share match_est / from_ref / match_ref, each class touching the
// entries of its own estimates and references only, and own one row of the queue each.
#pragma once
#include "common.h"
#include "event_records.h"

#pragma clang fp contract(off)     // the float64 collar tests must be the plain sub / mul / compare sed_eval evaluates

namespace sedt {

// every lane of the wave calls this (it votes): lane = estimate, `live` whether the lane holds one, (cls, on, end) its class and its
// float64 times.  A hit: same class, |on_r - on_e| <= t_collar, |off_r - off_e| <= max(t_collar, pct * (off_r - on_r)).
__device__ inline void event_hit_graph(unsigned long long* adj, const int* r_cls, const double* r_on, const double* r_end, int ne,
                                       bool live, int cls, double on, double end, double t_collar, double pct, int lane) {
  for (int j = 0; j < ne; ++j) {
    const double ron = r_on[j], rend = r_end[j];
    const double off_collar = fmax(t_collar, pct * (rend - ron));
    const bool hit = live && cls == r_cls[j] && fabs(ron - on) <= t_collar && fabs(rend - end) <= off_collar;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) adj[j] = m;
  }
}

// one lane per class: the references of class c in table order; returns tp and counts them into n_ref.  match_est[q] = -1 for every
// estimate and match_ref[j] = -1 for every reference on entry.  Greedy (optimal == 0): each reference takes the first estimate still
// free that it hits, the estimates tried in the order order[0 .. n_order) - or, with order == nullptr, in index order.
__device__ inline int event_class_match(int c, int ne, const int* r_cls, const unsigned long long* adj, int* match_est, int* from_ref,
                                        int* match_ref, unsigned char* qu, int optimal, const int* order, int n_order, long& n_ref) {
  int tp = 0;
  for (int j = 0; j < ne; ++j) {
    if (r_cls[j] != c) continue;
    ++n_ref;
    if (adj[j] == 0ull) continue;
    if (optimal) {
      int head = 0, tail = 0, found = -1;
      unsigned long long seen = 0ull;
      qu[tail++] = (unsigned char)j;
      while (head < tail && found < 0) {
        const int r = qu[head++];
        unsigned long long avail = adj[r] & ~seen;
        while (avail) {
          const int q = __ffsll((long long)avail) - 1;
          avail &= avail - 1ull;
          seen |= 1ull << q;
          from_ref[q] = r;
          if (match_est[q] < 0) { found = q; break; }
          qu[tail++] = (unsigned char)match_est[q];    // each matched ref enters once: its estimate is seen once
        }
      }
      if (found >= 0) {
        int q = found;
        for (;;) {                                      // flip the path back to j
          const int r = from_ref[q], prev = match_ref[r];
          match_ref[r] = q;
          match_est[q] = r;
          if (r == j) break;
          q = prev;
        }
        ++tp;
      }
    } else if (order) {
      for (int k = 0; k < n_order; ++k) {               // estimates in their output order, first free hit wins
        const int q = order[k];
        if (match_est[q] < 0 && ((adj[j] >> q) & 1ull)) {
          match_est[q] = j;
          ++tp;
          break;
        }
      }
    } else {
      for (unsigned long long avail = adj[j]; avail; avail &= avail - 1ull) {
        const int q = __ffsll((long long)avail) - 1;
        if (match_est[q] < 0) {
          match_est[q] = j;
          ++tp;
          break;
        }
      }
    }
  }
  return tp;
}

}  // namespace sedt
