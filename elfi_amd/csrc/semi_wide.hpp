// What the two wide semiparametric likelihoods share (semibsl_wide.hip: semiBSL of 65 to 256 summaries; wsemibsl_wide.hip:
// its whitened form): the arguments and the launches of the kernels that one file defines and the other one runs as well.
// The column kernel's are in semi_rank.hpp (SemiWideArgs, semibsl_launch_column_wide).
//   gram     semibsl_wide.hip.  SemiGramArgs: rho of the scores at Q, the lower blocks.  SemiCovArgs: the covariance of the
//            scores at Q (ddof 1) into R, every block, one value at (a, b) and (b, a); rho is not used.
//   finish   semibsl_wide.hip.  SemiWideFinArgs: the matrix (1 - l) rho + l I and eta.  WsemiWideFinArgs: the scaled matrix
//            diag(d) ((1 - l) rho + l I) diag(d) and eta_w, d and eta_w from the job's whitened statistics.
//   re-rank  wsemibsl.hip.  WsemiWideArgs: its wide layout, T and Q2 laid out as the wide Q.
#pragma once

#include "semi_rank.hpp"
#include "wide_chol.hpp"

namespace elfihip {

constexpr int SMW_RC = 32;             // rows per staged chunk of the gram kernel (8 MFMA steps)
constexpr int SMW_CP = SMW_RC + 2;     // pitch of a staged column

struct SemiGramArgs {
  const double* Q;          // (jobs, m, NP) of this launch
  const double* stats;      // (jobs, SEMI_WIDE_STATS)
  double* R;                // (jobs, mpad, mpad): rho, the lower blocks
  double* rho;              // (G, m, m) or NULL
  const int64_t* prefixes;  // (K)
  int64_t n, job0;          // job0: the launch's first job in the call, job = g K + k
  int m, mpad, NP, K, pairs;
};
struct SemiCovArgs : SemiGramArgs {};

struct SemiWideFinArgs {
  const double* R;          // (jobs, mpad, mpad) of the gram launch
  const double* stats;      // (jobs, SEMI_WIDE_STATS)
  double* slabs;            // one per workgroup
  double* loglik;           // (G, K, max(P, 1))
  const int64_t* prefixes;  // (K)
  const double* penalties;  // (P) or NULL
  int64_t job0;             // the gram launch's first job in the call
  int64_t fjob0;            // this launch's first (job, penalty), counted from the gram launch's first job
  int m, mpad, pw, K, P;
};
// The whitened statistics of a job, next to the column kernel's: d at 0, eta_w = W eta at SEMI_WIDE_M.
constexpr int WSEMI_WIDE_STATS = 2 * SEMI_WIDE_M;
struct WsemiWideFinArgs : SemiWideFinArgs {
  const double* wst;        // (jobs, WSEMI_WIDE_STATS)
};

struct WsemiWideArgs {
  SemiWideArgs S;    // the column kernel's arguments (its rho and scores NULL: the outputs below are of the transformed scores)
  const double* W;   // (m, m) row-major, pitch m
  double* T;         // (jobs, m, NP): the transformed scores, laid out as S.Q
  double* Q2;        // (jobs, m, NP): the scores of T's columns; may be T
  const double* C;   // (jobs, mpad, mpad): cov(Q), symmetric, zero beyond m
  double* wst;       // (jobs, WSEMI_WIDE_STATS)
  double* scale;     // (G, m) or NULL
  double* scores;    // (G, n, m) or NULL
  int chunks, nb, mpad;   // 64-row chunks of n rows; 64-column blocks of m columns
};

// Launches over `jobs` (group, prefix) jobs on the context's stream; the finish launches take `count` (job, penalty) pairs
// from F.fjob0 on.
int semibsl_wide_launch_gram(elfihip_ctx* ctx, const SemiGramArgs& M, int64_t jobs);
int semibsl_wide_launch_cov(elfihip_ctx* ctx, const SemiCovArgs& M, int64_t jobs);
int semibsl_wide_launch_finish(elfihip_ctx* ctx, const SemiWideFinArgs& F, int64_t count);
int semibsl_wide_launch_finish_scaled(elfihip_ctx* ctx, const WsemiWideFinArgs& F, int64_t count);
int wsemi_launch_rerank_wide(elfihip_ctx* ctx, const WsemiWideArgs& A, int64_t jobs);

}  // namespace elfihip
