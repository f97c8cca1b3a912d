// lsa_pose_graph.h -- the host statement of the pose-graph solve: graph validation, the poses' incidence lists, and the plain
// sequential Levenberg-Marquardt loop over ../lsa_pose_graph.h, the text the device compiles too (lsa_pose_graph.hip).  The
// tridiagonal preconditioner is solved by block Thomas here, by cyclic reduction on the device: the two agree to rounding,
// everything else (linearization, assembly) bit for bit.  No device, no state: a stand-alone program links it
// (tests/pose_graph_sanitize.cpp).
#pragma once
#include <string>
#include <vector>
#include "../lsa_pose_graph.h"

namespace lsa
{
namespace host
{
struct PoseGraph
{
  int n = 0, m = 0;
  std::vector<int> row_start, inc;                    // incidence lists, CSR, ascending edge index
  std::vector<int> loop_start, loop_edge, loop_col;   // couplings beyond the chain between free poses (pg::Graph)
  int k = 0;
  std::vector<int> prior_start, prior_of;             // the priors of the poses, CSR, ascending prior index
  pg::Graph view() const { return pg::Graph{row_start.data(), inc.data(), loop_start.data(), loop_edge.data(), loop_col.data(), prior_start.data(), prior_of.data()}; }
};
// LSA_E_ARG (and why) unless the graph is within the definition; fixed may be NULL where none is needed (linearization)
int PgoCheckEdges(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, std::string* why);
// priors: k of them behind one offset (offset16 may be NULL when k is 0); a graph needs a fixed pose or a prior
int PgoCheckPriors(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, std::string* why);
int PgoBuild(const double* poses16, int n, const unsigned char* fixed, const lsa_pgo_edge_t* edges, int m, PoseGraph* g, std::string* why,
             const lsa_pgo_prior_t* priors = nullptr, int k = 0, const double* offset16 = nullptr);
// block Thomas on the block-tridiagonal (D, L, U); false when a pivot block is not positive definite (x untouched)
bool PgoTridiagonalSolve(int n, const double* D, const double* L, const double* U, const double* b, double* x);
const char* PgoMessage(int termination);
int PgoSolve(const double* poses16, int n, const unsigned char* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k, const double* offset16,
             const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result, std::string* why, const unsigned char* edgeMask = nullptr,
             const lsa_pgo_robust_t* robust = nullptr, double* edgeVerdict = nullptr, double* priorVerdict = nullptr);  // the losses: ../lsa_pose_graph.h ROBUST LOSS
}  // namespace host
}  // namespace lsa
