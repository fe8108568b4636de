# Builds the gfx950 shared library (product), the CPU oracle (test infrastructure) and the host executable.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH ?= gfx950
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -munsafe-fp-atomics -Wall -Wno-unused-function $(EXTRA)
CSRC := xpic_amd/csrc
SRCS := $(CSRC)/api.hip $(CSRC)/fields.hip $(CSRC)/particles.hip $(CSRC)/ecsim.hip $(CSRC)/ecsim_ws.hip $(CSRC)/esirkepov.hip $(CSRC)/krylov.hip $(CSRC)/precond.hip $(CSRC)/comm.hip $(CSRC)/eccapfim.hip $(CSRC)/moments.hip $(CSRC)/commands.hip $(CSRC)/collide.hip $(CSRC)/drift_kinetic.hip $(CSRC)/full_orbit.hip $(CSRC)/trace_open.hip $(CSRC)/model_trace.hip $(CSRC)/collide_trace.hip $(CSRC)/background.hip $(CSRC)/compare_trace.hip $(CSRC)/tracers.hip $(CSRC)/field_lines.hip $(CSRC)/tracer_moments.hip $(CSRC)/gauss.hip $(CSRC)/es.hip $(CSRC)/poisson.hip $(CSRC)/spectrum.hip
OBJS := $(SRCS:.hip=.o)
HDRS := $(wildcard $(CSRC)/*.h) include/xpic_hip.h include/xpic_set_particles.h include/xpic_tracers.h include/xpic_tracer_moments.h include/xpic_field_lines.h include/xpic_gauss.h include/xpic_es.h include/xpic_poisson.h include/xpic_spectrum.h

all: xpic_amd/libxpic_hip.so xpic_amd/host/xpic_hip.out oracle

xpic_amd/libxpic_hip.so: $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -o $@ $(OBJS) -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib

$(CSRC)/%.o: $(CSRC)/%.hip $(HDRS)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

HOST := xpic_amd/host
xpic_amd/host/xpic_hip.out: $(HOST)/main.cpp $(HOST)/xpic_host.cpp $(HOST)/xpic_host.h $(HOST)/json.h include/xpic_hip.h include/xpic_set_particles.h include/xpic_tracers.h include/xpic_tracer_moments.h include/xpic_field_lines.h include/xpic_gauss.h include/xpic_es.h include/xpic_poisson.h include/xpic_spectrum.h xpic_amd/libxpic_hip.so
	g++ -O2 -std=c++17 -Wall -Wextra -o $@ $(HOST)/main.cpp $(HOST)/xpic_host.cpp -Lxpic_amd -lxpic_hip -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath-link,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

clean:
	rm -f $(OBJS) xpic_amd/libxpic_hip.so xpic_amd/host/xpic_hip.out
	$(MAKE) -C oracle clean

.PHONY: all oracle clean
