// Label-equivalence union-find of csrc/components.hip, written over a small "atomic" functor so that the same dozen lines run on the
// device (vector atomics on the workspace) and in a host program (std::atomic, several threads, or one thread in any pixel order).
//
//   A::load(i)      -> parent[i], read afresh (never a value kept in a register from an earlier read)
//   A::min(i, v)    -> atomically parent[i] = min(parent[i], v); returns the value that was there
//
// Invariant: every value ever stored in parent[i] is <= i, and parent[i] only decreases.  (Initially parent[i] <= i: the start of
// the pixel's run inside its 64-pixel segment.)
//
// Termination.
//   cc_find: every hop goes to a strictly smaller index (parent[i] < i unless i is a root) -- at most i hops, whatever other
//     threads store meanwhile, and whether the loads are fresh or stale.
//   cc_unite: an iteration that does not return ends with x = old < (the larger root of that iteration): the atomic found
//     parent[x] != x, so old < x.  The next pair of roots is (find(old), find(y)), both below the previous x.  The larger root of
//     the pair strictly decreases from one iteration to the next: at most (index of the first x) iterations.
// Result.
//   The atomic at the larger root x leaves parent[x] = min(old, y).  If old == x the root now hangs under y: done.  Otherwise x was
//   no root any more; whichever of old, y lost the minimum is not linked to x by this store, so the pair (old, y) still has to be
//   united -- the loop goes on from it.  Links are only ever replaced by the thread that takes over the obligation to restore
//   them, so when every thread has returned, any two pixels that were ever united have one root.  A root is <= all its members
//   and is one of them: it is the component's first pixel in raster order, whatever order the atomics landed in.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

template <class A> CC_HD int cc_find(A& a, int i) {
  for (;;) {
    const int p = a.load(i);
    if (p == i) return i;
    i = p;
  }
}

template <class A> CC_HD void cc_unite(A& a, int x, int y) {
  for (;;) {
    x = cc_find(a, x);
    y = cc_find(a, y);
    if (x == y) return;
    if (x < y) { const int t = x; x = y; y = t; }
    const int old = a.min(x, y);
    if (old == x) return;
    x = old;
  }
}

// The unions of pixel l = (z, y, x) of a row (cls, a: based at the row's first pixel; plane = H * W) with its already-visited
// neighbours of the same class.  seg_start: the pixel is the first of its 64-pixel segment (the initial parents chain runs only
// inside a segment).  A union is left out where the pair is connected through pairs that are united elsewhere:
//   up          when left and up-left are of the class too   (p - left: same run; left - up-left: left's own "up"; up-left - up: same run)
//   up-left     when left or up is of the class               (left - up-left / up - up-left are face neighbours)
//   up-right    when up is of the class
//   z - 1       when left and left's z - 1 are of the class too
//   the 8 others in slice z - 1 (full)   when the face neighbour in z - 1 is of the class: it touches all of them
// Each of these rests only on pairs whose later pixel comes before p, on p's own face pairs, or on runs: no circle.
template <class A>
CC_HD void cc_merge_pixel(A& a, const unsigned char* cls, int l, int x, int y, int z, int H, int W, int full, int method3d, bool seg_start) {
  const unsigned char c = cls[l];
  const bool L = x > 0 && cls[l - 1] == c;
  const bool U = y > 0 && cls[l - W] == c;
  const bool UL = x > 0 && y > 0 && cls[l - W - 1] == c;
  if (L && seg_start) cc_unite(a, l, l - 1);
  if (U && !(L && UL)) cc_unite(a, l, l - W);
  if (full) {
    if (UL && !L && !U) cc_unite(a, l, l - W - 1);
    if (!U && y > 0 && x < W - 1 && cls[l - W + 1] == c) cc_unite(a, l, l - W + 1);
  }
  if (method3d && z > 0) {
    const int plane = H * W;
    const unsigned char* q = cls + (l - plane);
    if (q[0] == c) {
      if (!(L && q[-1] == c)) cc_unite(a, l, l - plane);
    } else if (full) {
      for (int dy = -1; dy <= 1; ++dy) {
        if (y + dy < 0 || y + dy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          if (x + dx < 0 || x + dx >= W || (dx == 0 && dy == 0)) continue;
          if (q[dy * W + dx] == c) cc_unite(a, l, l - plane + dy * W + dx);
        }
      }
    }
  }
}
