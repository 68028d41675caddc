// The states of the SMILES grammar (decode.py grammar_step is the statement; the classes are GCT_GRAMMAR_*), shared by
// grammar_allows / grammar_mask_kernel (decode.hip), the chemistry check's walk (chem.hip) and rand_parse (smiles_graph.h).
#pragma once

namespace {

enum { GP_START = 0, GP_ATOM, GP_RING, GP_BOND_A, GP_BOND_B, GP_OPEN, GP_CLOSE, GP_DOT, GP_END };
constexpr int kNone = 0x7fffffff;                            // "no position", "no token"

}  // namespace
