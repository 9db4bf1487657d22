// The core of the connected-parts labelling (object_parts.hip), free of anything a GPU needs: the lock-free find and union over a parent array,
// the packed word that names a slot's largest part, and the keep rule.  Every function is __host__ __device__ and takes the memory it works on
// through a small policy (load / fetch_min on one int), so the kernels run it on LDS and on global memory with agent-scope atomics, and a plain
// host program (tools/parts_host_check.cpp) replays the same phases one after the other on ordinary memory, under a sanitizer.
//
// The parent array: parent[i] <= i for every i, a root has parent[i] == i.  A union hooks the LARGER root under the smaller one with an integer
// minimum, so parents only ever decrease and the root of a finished set is its smallest index -- the part's name, with no renumbering pass.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PT_HD __host__ __device__ __forceinline__
#else
#define PT_HD inline
#endif

// status bits of a frame: a bounded loop gave up
#define PT_GAVE_UP_LOCAL 1
#define PT_GAVE_UP_SEAM 2
#define PT_GAVE_UP_FLATTEN 4

// plain memory: the host program, and phases in which no other workgroup writes the words read
struct PtPlain {
  PT_HD static int load(const int* p) { return *p; }
  PT_HD static int fetch_min(int* p, int v) { const int old = *p; if (v < old) *p = v; return old; }
};

// The root of i.  Every step goes to a strictly smaller index (parent[x] < x for a non-root), so a walk from i ends after at most i steps;
// `cap` is that bound for the array at hand (its length): *gave_up is set, and the walk left where it stands, when it is reached.
// A walk of three steps or more shortens the next ones: the node it visited first (for a pixel: the root of its part inside its tile, which
// every pixel of that part in the tile passes) is pointed at the root found, by fetch_min -- the root is an ancestor of that node and smaller
// than its parent, so parents still only decrease and no set changes.
template <class M>
PT_HD int pt_find(int* parent, int i, int cap, bool* gave_up) {
  int x = i, first = i;
  for (int t = 0; t <= cap; ++t) {
    const int up = M::load(parent + x);
    if (up == x) {
      if (t >= 3) M::fetch_min(parent + first, x);
      return x;
    }
    if (t == 0) first = up;
    x = up;
  }
  *gave_up = true;
  return x;
}

// Joins the sets of a and b.  Find both roots; hook the larger under the smaller with fetch_min on parent[larger].  The value returned tells
// whether the larger one still was a root: if not, another union got there first -- its set now hangs under `old` (or, where the minimum took
// effect, under both `old` and the smaller root, which is why the walk continues from `old`: nothing is lost).  Every round but the last
// replaces a or b by a strictly smaller index, so there are at most a + b <= 2 cap rounds; with the finds inside, `cap` bounds each.
template <class M>
PT_HD void pt_union(int* parent, int a, int b, int cap, bool* gave_up) {
  for (int t = 0; t <= 2 * cap; ++t) {
    a = pt_find<M>(parent, a, cap, gave_up);
    b = pt_find<M>(parent, b, cap, gave_up);
    if (a == b || *gave_up) return;
    if (a < b) { const int c = a; a = b; b = c; }                       // a: the larger root
    const int old = M::fetch_min(parent + a, b);
    if (old == a) return;                                               // a was a root and now hangs under b
    a = old;
  }
  *gave_up = true;
}

// (area, name) of a part as one word whose unsigned maximum is the largest part, ties to the smaller name; 0: no part.  area <= 2^28, name < 2^28.
PT_HD unsigned long long pt_pack(int area, int name) { return ((unsigned long long)(unsigned)area << 32) | (unsigned)(0x7fffffff - name); }
PT_HD int pt_packed_area(unsigned long long v) { return (int)(v >> 32); }
PT_HD int pt_packed_name(unsigned long long v) { return v == 0 ? -1 : 0x7fffffff - (int)(v & 0xffffffffu); }

// Is the part `name` of `area` pixels kept?  `ruled`: its slot's id differs from fill; `largest`: the name of its slot's largest part.
PT_HD bool pt_keep(bool ruled, int area, int name, int largest, long long min_area, bool largest_only) {
  return !ruled || ((long long)area >= min_area && (!largest_only || name == largest));
}
