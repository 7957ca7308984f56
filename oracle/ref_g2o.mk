# oracle/_ref/libg2o_ref.so: the reference's own g2o core (SparseOptimizer, BlockSolver_6_3,
# LinearSolverEigen over its bundled Eigen, Levenberg, the terminate action, the Huber kernel)
# compiled from the reference checkout and linked with oracle/ref_g2o_driver.cpp.
#
# TEST INFRASTRUCTURE ONLY.  Run from oracle/ (`make -f ref_g2o.mk -j8`); a no-op without the
# checkout.  Nothing under _ref/ is committed.  This file names paths only.
REF      ?= /root/reference
G2O      := $(REF)/ThirdParty/g2o
EIGEN    := $(REF)/ThirdParty/Eigen
OUT      := _ref
INC      := $(OUT)/include
# no contraction, no -march: the project's convention for everything a fixture is made with
FLAGS    := -O2 -fPIC -ffp-contract=off -fno-fast-math -DNDEBUG -w
CXXFLAGS := -std=gnu++14 $(FLAGS)
# "../../config.h" (core/openmp_mutex.h) resolves through $(INC)/a/b, "config.h" through $(INC)
INCLUDES := -I$(INC) -I$(INC)/a/b -I$(G2O) -I$(EIGEN)

CORE_SRC  := $(filter-out %/sparse_block_matrix_test.cpp,$(wildcard $(G2O)/g2o/core/*.cpp))
STUFF_SRC := $(wildcard $(G2O)/g2o/stuff/*.cpp)
STUFF_C   := $(G2O)/g2o/stuff/os_specific.c
OBJS := $(patsubst $(G2O)/g2o/core/%.cpp,$(OUT)/obj/core_%.o,$(CORE_SRC)) \
        $(patsubst $(G2O)/g2o/stuff/%.cpp,$(OUT)/obj/stuff_%.o,$(STUFF_SRC)) \
        $(OUT)/obj/stuff_os_specific_c.o $(OUT)/obj/ref_g2o_driver.o $(OUT)/obj/ba_oracle.o

ifeq ($(wildcard $(G2O)/g2o/core/sparse_optimizer.cpp),)
all:
	@echo "ref_g2o.mk: no reference checkout at $(REF); nothing to build"
else
all: $(OUT)/libg2o_ref.so
endif

$(INC)/config.h:
	mkdir -p $(INC)/a/b $(OUT)/obj
	printf '%s\n' '#ifndef MCS_REF_G2O_CONFIG_H' '#define MCS_REF_G2O_CONFIG_H' \
	  '/* written by oracle/ref_g2o.mk: no OpenMP, no CHOLMOD, no CSparse, no OpenGL */' \
	  '#ifdef __cplusplus' '#include <g2o/core/eigen_types.h>' '#endif' '#endif' > $@

$(OUT)/obj/core_%.o: $(G2O)/g2o/core/%.cpp $(INC)/config.h
	$(CXX) $(CXXFLAGS) $(INCLUDES) -c $< -o $@
$(OUT)/obj/stuff_%.o: $(G2O)/g2o/stuff/%.cpp $(INC)/config.h
	$(CXX) $(CXXFLAGS) $(INCLUDES) -c $< -o $@
$(OUT)/obj/stuff_os_specific_c.o: $(STUFF_C) $(INC)/config.h
	$(CC) $(FLAGS) $(INCLUDES) -c $< -o $@
$(OUT)/obj/ref_g2o_driver.o: ref_g2o_driver.cpp ../include/mcs_ba.h $(INC)/config.h
	$(CXX) $(CXXFLAGS) $(INCLUDES) -c $< -o $@
# the edge's error and Jacobian (oracle_ba_edge) are compiled in, so the library stands alone
$(OUT)/obj/ba_oracle.o: ba_oracle.cpp ../include/mcs_ba.h $(INC)/config.h
	$(CXX) -std=c++17 $(FLAGS) -c $< -o $@

$(OUT)/libg2o_ref.so: $(OBJS)
	$(CXX) -shared -o $@ $(OBJS)

.PHONY: all
