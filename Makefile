# Build libqcart.so (HIP, gfx950) in-tree and the CPU oracle (test infrastructure).
HIPCC ?= /opt/rocm/bin/hipcc
PKG := deepreinforcementlearningcontrolofquantumcartpoles_amd
CSRC := $(PKG)/csrc
LIB := $(PKG)/libqcart.so
# -ffp-contract=on: a * b + c is fused where the source writes it as one expression and nowhere else, so
# every instantiation of a step body (table placements, single- and two-slot workgroups) does bit-identical
# arithmetic; an env's trajectory never depends on which workgroup shape it ran in (the backend's "fast"
# contraction fused differently per instantiation)
HIPFLAGS ?= -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -ffp-contract=on
OBJS := $(addprefix $(CSRC)/build/,qcart_k_ho.o qcart_k_iho.o qcart_k_grid.o qcart_k_f32.o qcart_k_group.o qcart_record.o qcart_noise.o qcart_replay.o qcart_actor.o qcart_learner.o qcart_mlearner.o qcart_dispatch.o qcart_api.o qcart_tables.o qcart_server.o qcart_env.o qcart_sched.o qcart_monitor.o qcart_spatial.o qcart_wigner.o qcart_ensemble.o qcart_levels.o qcart_lindblad.o qcart_phase.o qcart_filter.o)
HDRS := include/qcart.h $(CSRC)/qcart_mt.hpp $(CSRC)/qcart_expt.hpp $(CSRC)/qcart_kargs.hpp $(CSRC)/qcart_tables.hpp $(CSRC)/qcart_kernels.hpp $(CSRC)/qcart_mfma.hpp $(CSRC)/qcart_dqn.hpp $(CSRC)/qcart_host.hpp $(CSRC)/qcart_learner.hpp $(CSRC)/qcart_state.hpp $(CSRC)/qcart_sched.hpp $(CSRC)/qcart_monitor.hpp $(CSRC)/qcart_spatial.hpp $(CSRC)/qcart_wigner.hpp $(CSRC)/qcart_ensemble.hpp $(CSRC)/qcart_levels.hpp $(CSRC)/qcart_lindblad.hpp $(CSRC)/qcart_phase.hpp $(CSRC)/qcart_filter.hpp $(CSRC)/qcart_wigner_tiles.hpp $(CSRC)/qcart_shm.h
# the step server's client side: plain C (POSIX shared memory + futexes), no HIP
CLIENT := $(PKG)/libqcart_client.so

all: $(LIB) $(CLIENT) oracle

$(CLIENT): $(CSRC)/qcart_client.c $(CSRC)/qcart_shm.h include/qcart_client.h Makefile
	gcc -O2 -std=gnu11 -fPIC -shared -Wall -o $@ $< -lrt -lm

# kernel TUs: MachineLICM off — it hoists loop-invariant FP64 constants of the step loop's rare
# noise refill into registers that then spill (same speed, ~0.9 GB less scratch traffic per launch)
KFLAGS ?= -mllvm -disable-machine-licm
# (the grid TU keeps LICM: its 9-band loop-invariant addressing is worth hoisting, measured +12 %; and
# contracts across statements: C3 -3 % against -ffp-contract=on, its table placements and two-slot
# workgroups still bit-identical — tests/test_gpu_parity.py checks both; "fast-honor-pragmas": the same code for every
# step / observation kernel, but the backend fuses only what the front end marked, so the math library's code and
# the Box–Muller under `fp contract(on)` (qcart_mt.hpp, the resident kernel) round as in the other TUs — only the
# Gaussian-packet reset kernels' exp changed, by the library's own contraction); the scheduler with the AMDGPU register
# pressure trackers: C3's R = 17 kernel 418 -> 400 VGPRs, 157.2 -> 150.0 ms per launch (alternating A/B pairs;
# the metric, C2 and C5 TUs were measured unchanged with it and keep the default)
$(CSRC)/build/qcart_k_grid.o: KFLAGS := -ffp-contract=fast-honor-pragmas -mllvm -amdgpu-use-amdgpu-trackers
# fp32 TU: complex values as packed 2-lane vectors (QCART_F32_PACKED, explicit v_pk_* arithmetic; MS property
# accessors keep .re/.im) and no SLP packing of the remaining scalar code (it would reshuffle the pairs)
$(CSRC)/build/qcart_k_f32.o: KFLAGS += -fno-slp-vectorize -fms-extensions -DQCART_F32_PACKED
$(CSRC)/build/%.o: $(CSRC)/%.hip $(HDRS) Makefile
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) -c $< -o $@
$(CSRC)/build/%.o: $(CSRC)/%.cpp $(HDRS) Makefile
	@mkdir -p $(CSRC)/build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) $(HIPFLAGS) -shared -o $@ $^ -lrt

oracle:
	$(MAKE) -C oracle

clean:
	rm -rf $(CSRC)/build $(LIB) $(CLIENT)
	$(MAKE) -C oracle clean

.PHONY: all oracle clean resource-usage expt expt_actor

# experiment builds (not shipped): make expt EXPT=-DQCART_STAMPS NAME=stamps [TU=qcart_k_grid]
EXPT ?=
NAME ?= expt
TU ?= qcart_k_iho
expt: $(OBJS)
	@mkdir -p $(CSRC)/build_$(NAME)
	$(HIPCC) $(HIPFLAGS) $(if $(filter qcart_k_grid,$(TU)),-ffp-contract=fast-honor-pragmas -mllvm -amdgpu-use-amdgpu-trackers,$(KFLAGS)) $(if $(filter qcart_k_f32,$(TU)),-fno-slp-vectorize -fms-extensions -DQCART_F32_PACKED,) $(EXPT) -c $(CSRC)/$(TU).hip -o $(CSRC)/build_$(NAME)/$(TU).o
	$(HIPCC) $(HIPFLAGS) -shared -o $(PKG)/libqcart_$(NAME).so $(CSRC)/build_$(NAME)/$(TU).o $(filter-out $(CSRC)/build/$(TU).o,$(OBJS))
# actor experiment builds: make expt_actor EXPT='-DQCART_MCONV_Q=4' NAME=q4
expt_actor:
	@mkdir -p $(CSRC)/build_$(NAME)
	$(HIPCC) $(HIPFLAGS) $(KFLAGS) $(EXPT) -c $(CSRC)/qcart_actor.hip -o $(CSRC)/build_$(NAME)/qcart_actor.o
	$(HIPCC) $(HIPFLAGS) -shared -o $(PKG)/libqcart_$(NAME).so $(CSRC)/build_$(NAME)/qcart_actor.o $(filter-out $(CSRC)/build/qcart_actor.o,$(OBJS))
