// What the Krylov solvers (krylov.hip) see of the handles that stand in for the matrix: of a domain handle
// (mimi_hip_linear_set_operator) its size and device and the tangent action launched on the SOLVER's stream -- defined in
// domain.hip, the kernels are kernels_apply.hpp; of a contact or follower-pressure handle
// (mimi_hip_linear_add_boundary_operator) the same for the action of its face tangent -- defined in contact.hip and
// pressure.hip, the kernels are kernels_face_action.hpp; of a periodic fold (mimi_hip_linear_set_operator_fold) its node
// map and copies table -- defined in fold.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct mimi_hip_domain_s;
struct mimi_hip_contact_s;
struct mimi_hip_pressure_s;
struct mimi_hip_fold_s;

namespace mimi_hip {

int64_t operator_size(const mimi_hip_domain_s* h);
int operator_device(const mimi_hip_domain_s* h);
// once per solve: the checks of mimi_hip_domain_apply_tangent, whatever the action builds on first use (finished before it
// returns), and one wait of solver_stream on the event recorded behind the last mimi_hip_domain_linearize
void operator_begin_solve(mimi_hip_domain_s* h, double density, double stiffness, hipStream_t solver_stream);
// y += density M x + stiffness K x + viscosity C x; x, y on the device, everything on solver_stream
void operator_add_action(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, const double* x, double* y,
                         hipStream_t solver_stream);

// The diagonal of the same operator (mimi_hip_domain_tangent_diagonal).  begin_diagonal, once per solve behind begin_solve:
// the checks and what the diagonal kernels build on first use (the element pieces of `block`); add_diagonal: d += the diagonal
// (block == 0: [A][i]) or the node blocks (block != 0: [A][i][j]); d on the device, everything on solver_stream.
int operator_dim(const mimi_hip_domain_s* h);
void operator_begin_diagonal(mimi_hip_domain_s* h, double density, double stiffness, int block, hipStream_t solver_stream);
void operator_add_diagonal(mimi_hip_domain_s* h, double density, double stiffness, double viscosity, int block, double* d,
                           hipStream_t solver_stream);

// The boundary twins.  begin_solve: the check of mimi_hip_<kind>_apply_tangent (a linearize came first), the face vector of
// the action, and one wait of solver_stream on the event recorded behind the handle's last linearize.
// add_action: y += factor K_face x; x, y on the device, everything on solver_stream.
int64_t operator_size(const mimi_hip_contact_s* h);
int operator_device(const mimi_hip_contact_s* h);
void operator_begin_solve(mimi_hip_contact_s* h, hipStream_t solver_stream);
void operator_add_action(mimi_hip_contact_s* h, double factor, const double* x, double* y, hipStream_t solver_stream);
int64_t operator_size(const mimi_hip_pressure_s* h);
int operator_device(const mimi_hip_pressure_s* h);
void operator_begin_solve(mimi_hip_pressure_s* h, hipStream_t solver_stream);
void operator_add_action(mimi_hip_pressure_s* h, double factor, const double* x, double* y, hipStream_t solver_stream);

// Of a periodic fold (mimi_hip_linear_set_operator_fold) the tables it built at create, read in place by the folded product
// of krylov.hip -- defined in fold.hip.  node_map[n_nodes_u] -> folded node; the copies of folded node F are
// copies[copy_ptr[F] .. copy_ptr[F + 1]), ascending: the order in which the fold adds the residual's source rows.
struct OperatorFold {
  int dim;
  int64_t n_nodes_u, n_nodes_f;
  const int32_t* node_map;
  const int32_t* copy_ptr;
  const int32_t* copies;
};
int operator_device(const mimi_hip_fold_s* h);
OperatorFold operator_fold(const mimi_hip_fold_s* h);

}  // namespace mimi_hip
