# The rules of every library's Makefile, stated once.  A Makefile sets OUT (the shared object) and DEPS (the prerequisites outside
# its directory, relative to it) and includes this file; make -C <directory> builds that library alone.  Every object depends on
# its source, on every header of its directory, on DEPS and on the two .mk files.
include ../csrc/flags.mk
SRCS    := $(wildcard *.hip)
OBJS    := $(SRCS:%.hip=_obj/%.o)

all: $(OUT)

_obj/%.o: %.hip ../csrc/flags.mk ../csrc/rules.mk $(wildcard *.h) $(DEPS)
	@mkdir -p _obj
	$(HIPCC) $(CXXFLAGS) $(EXTRA) -c $< -o $@

$(OUT): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)

clean:
	rm -rf _obj $(OUT)
.PHONY: all clean
