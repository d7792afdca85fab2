# The compiler, the target and the compile flags of every library, stated once: the bit-for-bit contracts between them
# (-ffp-contract=off, the correctly rounded divide and sqrt) rest on every object being compiled alike.
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CXXFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt \
            -Wall -Wno-unused-function
