/* ----------------------------------------------------------------------
   pair_style e3gnn/parallel on MI355X (see pair_e3gnn_parallel_hip.h).

   Reference: sevenn/pair_e3gnn/pair_e3gnn_parallel.cpp -- compute (:207-541),
   coeff (:560-690), init_style (:693-699), comm_preprocess (:703-748),
   pack_/unpack_forward_init (:750-801), pack_/unpack_{forward,reverse}_comm_gnn
   (:803-933).  The graph build, the per-layer segment calls and the force /
   virial / eatom scatter are e3gnn_pair::ParallelStep (native/pair_e3gnn_core.cpp);
   the per-swap row maps of the "false" preprocessing forward_comm and their
   reverse dedup are e3gnn_pair::CommMaps (tested under an in-process CommBrick
   emulation, native/e3gnn_pair_check.cpp); this file only maps the CommBrick
   hooks onto them and moves the rows into / out of the MPI buffers (device
   buffers with GPU-aware MPI, host-staged otherwise).
------------------------------------------------------------------------- */

#include "pair_e3gnn_parallel.h"

#include "atom.h"
#include "comm.h"
#include "comm_brick.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "memory.h"
#include "neigh_list.h"
#include "neighbor.h"

#include "e3gnn.h"
#include "pair_e3gnn_core.h"

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <stdexcept>

using namespace LAMMPS_NS;

// the core's exchange = LAMMPS' patched brick communication
struct PairE3GNNParallel::Exchange : e3gnn_pair::ParallelStep::Exchange {
  PairE3GNNParallel *pair;
  CommBrick *brick;
  int forward(e3gnn_pair::ParallelStep &) override
  {
    brick->forward_comm(pair);
    return 0;
  }
  int reverse(e3gnn_pair::ParallelStep &) override
  {
    brick->reverse_comm(pair);
    return 0;
  }
};

PairE3GNNParallel::PairE3GNNParallel(LAMMPS *lmp) : Pair(lmp)
{
  single_enable = 0;
  restartinfo = 0;
  one_coeff = 1;
  manybody_flag = 1;
  // vatom is the edge-gradient partition of the virial (e3gnn_atom_virial);
  // a message-passing model has no centroid form of it
  centroidstressflag = CENTROID_NOTAVAIL;
  world_rank = comm->me;
  int ngpu = 1;
  if (hipGetDeviceCount(&ngpu) != hipSuccess || ngpu < 1) ngpu = 1;
  device = comm->me % ngpu;   // pair_e3gnn_parallel.cpp:153-189
  const char *env = std::getenv("OFF_E3GNN_PARALLEL_CUDA_MPI");
  use_cuda_mpi = !(env && std::strcmp(env, "1") == 0) && std::getenv("E3GNN_GPU_AWARE_MPI");
  if (hipSetDevice(device) != hipSuccess) error->one(FLERR, "e3gnn/parallel: hipSetDevice failed");
}

PairE3GNNParallel::~PairE3GNNParallel()
{
  maps.reset();
  if (d_stage) (void) hipFree(d_stage);
  if (allocated) {
    memory->destroy(setflag);
    memory->destroy(cutsq);
  }
}

int PairE3GNNParallel::get_x_dim() { return step && step->comm_dim() ? step->comm_dim() : comm_forward; }
bool PairE3GNNParallel::use_cuda_mpi_() { return use_cuda_mpi; }
bool PairE3GNNParallel::is_comm_preprocess_done() { return comm_preprocess_done; }

void PairE3GNNParallel::compute(int eflag, int vflag)
{
  ev_init(eflag, vflag);
  if (atom->tag_consecutive() == 0) error->all(FLERR, "Pair e3gnn requires consecutive atom IDs");
  CommBrick *brick = dynamic_cast<CommBrick *>(comm);
  if (!brick)
    error->all(FLERR, "e3gnn/parallel: comm style should be brick & from modified code of comm_brick");

  const int ntotal = atom->nlocal + atom->nghost;
  tag64.resize(ntotal);
  for (int i = 0; i < ntotal; i++) tag64[i] = atom->tag[i];
  e3gnn_pair::NeighborView nv;
  nv.inum = list->inum;
  nv.ilist = list->ilist;
  nv.numneigh = list->numneigh;
  nv.firstneigh = list->firstneigh;
  nv.x = atom->x;
  nv.type = atom->type;
  nv.tag = tag64.data();
  nv.nlocal = atom->nlocal;
  nv.nghost = atom->nghost;
  nv.neighmask = NEIGHMASK;
  nv.list_age = neighbor->ago;   // 0 on the step the list was rebuilt
  nv.x_flat = atom->x[0];        // Atom's x is one contiguous block (memory->create)
  // graph: local rows in list order, ghosts within the cutoff deduplicated by tag
  if (step->build(nv, species, atom->natoms)) error->one(FLERR, "e3gnn/parallel: " + step->error());
  comm_preprocess();

  Exchange ex;
  ex.pair = this;
  ex.brick = brick;
  e3gnn_pair::PairOut out;
  if (step->compute(ex, atom->f, eflag_atom ? eatom : nullptr, out, vflag_atom ? vatom : nullptr))
    error->one(FLERR, "e3gnn/parallel: " + step->error());
  eng_vdwl += out.energy;   // rank-local; LAMMPS sums over ranks
  if (vflag) for (int k = 0; k < 6; k++) virial[k] += out.virial[k];
  // ghost forces go to their owners with LAMMPS' reverse communication (newton
  // on), and so do the ghost rows of vatom (compute stress/atom's reverse_comm)
  comm_preprocess_done = false;
}

// ---------------------------------------------------------------- comm maps
// the "false" forward communication: CommBrick calls the *_init hooks per
// swap, e3gnn_pair::CommMaps keeps the row maps and their dedup (:703-748)
void PairE3GNNParallel::comm_preprocess()
{
  maps->begin();
  comm_preprocess_done = false;
  dynamic_cast<CommBrick *>(comm)->forward_comm(this);
  if (maps->finish()) error->one(FLERR, "e3gnn/parallel: " + maps->error());
  comm_preprocess_done = true;
}

void PairE3GNNParallel::pack_forward_init(int n, int *list_send, int comm_phase)
{
  if (maps->pack_forward_init(n, list_send, comm_phase)) error->one(FLERR, maps->error());
}

void PairE3GNNParallel::unpack_forward_init(int n, int first, int comm_phase)
{
  if (maps->unpack_forward_init(n, first, comm_phase)) error->one(FLERR, maps->error());
}

int PairE3GNNParallel::host_stage(int64_t floats)
{
  if (floats > stage_cap) {
    if (d_stage) (void) hipFree(d_stage);
    stage_cap = floats + floats / 4 + 1024;
    if (hipMalloc(&d_stage, stage_cap * 4) != hipSuccess) return 1;
  }
  return 0;
}

// the row copies run on device buffers: the MPI buffer itself with GPU-aware
// MPI, else the device staging buffer copied to / from the host buffer
int PairE3GNNParallel::gnn_copy(int which, float *buf, int comm_phase)
{
  const bool to_buf = which == 0 || which == 2;
  const int64_t n = (which == 0 || which == 3) ? maps->nsend(comm_phase) : maps->nrecv(comm_phase);
  const int64_t floats = n * step->comm_dim();
  if (!n) return 0;
  hipStream_t s = (hipStream_t) step->stream();
  float *dev = buf;
  if (!use_cuda_mpi) {
    if (host_stage(floats)) error->one(FLERR, "e3gnn/parallel: staging");
    dev = d_stage;
    if (!to_buf && hipMemcpyAsync(dev, buf, floats * 4, hipMemcpyHostToDevice, s) != hipSuccess)
      error->one(FLERR, "e3gnn/parallel: hipMemcpy");
  }
  int64_t rc = 0;
  switch (which) {
    case 0: rc = maps->pack_forward(comm_phase, dev); break;
    case 1: rc = maps->unpack_forward(comm_phase, dev); break;
    case 2: rc = maps->pack_reverse(comm_phase, dev); break;
    default: rc = maps->unpack_reverse(comm_phase, dev); break;
  }
  if (rc < 0) error->one(FLERR, "e3gnn/parallel: " + step->error());
  if (!use_cuda_mpi && to_buf && hipMemcpyAsync(buf, dev, floats * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
    error->one(FLERR, "e3gnn/parallel: hipMemcpy");
  if (hipStreamSynchronize(s) != hipSuccess) error->one(FLERR, "e3gnn/parallel: hipStreamSynchronize");
  return (int) floats;
}

int PairE3GNNParallel::pack_forward_comm_gnn(float *buf, int comm_phase)
{
  return gnn_copy(0, buf, comm_phase);
}

void PairE3GNNParallel::unpack_forward_comm_gnn(float *buf, int comm_phase)
{
  gnn_copy(1, buf, comm_phase);
}

int PairE3GNNParallel::pack_reverse_comm_gnn(float *buf, int comm_phase)
{
  return gnn_copy(2, buf, comm_phase);
}

void PairE3GNNParallel::unpack_reverse_comm_gnn(float *buf, int comm_phase)
{
  gnn_copy(3, buf, comm_phase);
}

// ---------------------------------------------------------------- setup
void PairE3GNNParallel::allocate()
{
  allocated = 1;
  const int n = atom->ntypes;
  memory->create(setflag, n + 1, n + 1, "pair:setflag");
  memory->create(cutsq, n + 1, n + 1, "pair:cutsq");
}

// pair_style e3gnn/parallel [graph host|device]: where the rank graph is built
// (e3gnn_pair::ParallelStep::GraphBuild; host when absent)
void PairE3GNNParallel::settings(int narg, char **arg)
{
  if (narg == 0) graph_device = 0;
  else if (narg == 2 && strcmp(arg[0], "graph") == 0 && strcmp(arg[1], "host") == 0) graph_device = 0;
  else if (narg == 2 && strcmp(arg[0], "graph") == 0 && strcmp(arg[1], "device") == 0) graph_device = 1;
  else error->all(FLERR, "Illegal pair_style command");
  if (step) step->set_graph_build(graph_device ? e3gnn_pair::ParallelStep::GraphBuild::Device
                                               : e3gnn_pair::ParallelStep::GraphBuild::Host);
}

// pair_coeff * * <n segments> <deployment dir> <element per type>: the
// reference reads one TorchScript file per segment (:578-608); one deployment
// directory holds every segment here (the segment API cuts at the same layer
// boundaries), so the count is accepted and not needed
void PairE3GNNParallel::coeff(int narg, char **arg)
{
  if (allocated) error->all(FLERR, "pair_e3gnn coeff called twice");
  allocate();
  if (narg < 4 || strcmp(arg[0], "*") != 0 || strcmp(arg[1], "*") != 0)
    error->all(FLERR, "e3gnn: first and second input of pair_coeff should be '*'");
  const int chem0 = 4;
  std::vector<std::string> elements;
  for (int i = chem0; i < narg; i++) elements.emplace_back(arg[i]);
  if (atom->ntypes > (int) elements.size())
    error->all(FLERR, "Not enough chemical specie is given. Check pair_coeff and types in your data/script");
  try {
    model.reset(new e3gnn_pair::Model(arg[3], device));
    species = model->type_map(elements);
    step.reset(new e3gnn_pair::ParallelStep(*model));
    if (graph_device) step->set_graph_build(e3gnn_pair::ParallelStep::GraphBuild::Device);
    maps.reset(new e3gnn_pair::CommMaps(*step));
  } catch (const std::exception &e) {
    error->all(FLERR, std::string("e3gnn/parallel: ") + e.what());
  }
  cutoff = model->cutoff();
  // per-atom floats exchanged between layers: the buffers CommBrick sizes (:619-624)
  comm_forward = model->comm_size();
  comm_reverse = model->comm_size();
  for (int i = 1; i <= atom->ntypes; i++)
    for (int j = 1; j <= atom->ntypes; j++) {
      setflag[i][j] = 1;
      cutsq[i][j] = cutoff * cutoff;
    }
}

void PairE3GNNParallel::init_style()
{
  // full neighbour list & newton on (:693-699)
  if (force->newton_pair == 0) error->all(FLERR, "Pair style e3gnn/parallel requires newton pair on");
  neighbor->add_request(this, NeighConst::REQ_FULL);
}

double PairE3GNNParallel::init_one(int, int) { return cutoff; }

// ---------------------------------------------------------------- device buffers
DeviceBuffManager &DeviceBuffManager::getInstance()
{
  // one per thread: one rank per process in LAMMPS, one per thread in the
  // in-process CommBrick emulation of native/e3gnn_pair_check
  static thread_local DeviceBuffManager instance;
  return instance;
}

void DeviceBuffManager::get_buffer(int send_size, int recv_size, float *&send, float *&recv)
{
  if (send_size > send_cap) {
    if (send_dev) (void) hipFree(send_dev);
    send_cap = send_size;
    if (hipMalloc(&send_dev, (size_t) send_cap * sizeof(float)) != hipSuccess) send_dev = nullptr;
  }
  if (recv_size > recv_cap) {
    if (recv_dev) (void) hipFree(recv_dev);
    recv_cap = recv_size;
    if (hipMalloc(&recv_dev, (size_t) recv_cap * sizeof(float)) != hipSuccess) recv_dev = nullptr;
  }
  send = send_dev;
  recv = recv_dev;
}

DeviceBuffManager::~DeviceBuffManager()
{
  if (send_dev) (void) hipFree(send_dev);
  if (recv_dev) (void) hipFree(recv_dev);
}
