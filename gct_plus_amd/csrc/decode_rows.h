// The row-slot rule of a decode step, stated once.  Every row of a step shares one device counter; `step` is the shared
// column the kernel works on -- *pos for the token the step consumes (embedding, attention), *pos + 1 for the token it
// chooses (grammar mask, selection, log-probability):
//   row r sits at column step - row_off[r]     (row_off null: 0 -- a batch of prefixes of different lengths otherwise)
//   a streamed row works on pool item item[r]  (item null: the row is its own item)
//   item < 0: the row is parked                (it touches nothing)
//   pos < prefix_len[item]: inside the prefix  (the slot keeps the token the refill laid there)
// The helper returns these facts; each kernel keeps its own bounds checks and early returns.  ragged / stream say
// whether row_off / item and prefix_len are in use: a template flag of the kernel (the branch folds away) or a null
// test of the pointer at run time.
#pragma once
#include <stdint.h>

struct GctRowSlot {
  int pos;   // the row's own column
  int item;  // the pool item of a streamed row (< 0: parked), the row itself otherwise
  int t0;    // the item's prefix length (0: plain or parked row)
  __device__ __forceinline__ bool acts() const { return item >= 0 && pos >= t0; }   // not parked, behind the prefix
};

__device__ __forceinline__ GctRowSlot gct_row_slot(int step, int row, bool ragged, const int32_t* row_off,
                                                   bool stream = false, const int32_t* item = nullptr,
                                                   const int32_t* prefix_len = nullptr) {
  GctRowSlot s;
  s.pos = ragged ? step - row_off[row] : step;
  s.item = stream ? item[row] : row;
  s.t0 = stream && s.item >= 0 ? prefix_len[s.item] : 0;
  return s;
}
