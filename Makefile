# lws-amd developer targets (reference Makefile analogue)
PY ?= python3

.PHONY: build test test-integration test-e2e test-gpu bench bench-full bench-ds smoke lint plan-steps manager clean

build:          ## build the gfx950 HIP kernel extension in-tree
	$(PY) -m lws_amd.ops.build

test:           ## CPU test tier (control plane, engine reference path, gloo TP)
	$(PY) -m pytest tests -q -m "not gpu"

test-integration:  ## in-process cluster tier (fake-runtime agents; envtest analogue)
	$(PY) -m pytest tests/test_lws_create.py tests/test_rolling_update.py \
	    tests/test_disaggregatedset.py tests/test_gang_scheduling.py \
	    tests/test_webhook_behaviors.py tests/test_events_and_resume.py -q

test-e2e:       ## subprocess manager + HTTP client + lwsctl (kind-e2e analogue)
	$(PY) -m pytest tests/test_manager_e2e.py tests/test_serving_server.py \
	    tests/test_serving_tp_cpu.py tests/test_durable_store.py \
	    tests/test_apiserver_auth.py tests/test_watch.py \
	    tests/test_subprocess_runtime.py tests/test_packaging.py -q -m "not gpu"

test-gpu:       ## MI355X tier (kernel numerics vs fp32 reference, HIP engine)
	$(PY) -m pytest tests -q -m gpu

bench:          ## flagship benchmark (BASELINE.json metric), 1 GPU
	$(PY) bench.py --gpus 1 --steps 3 --warmup 1

bench-full:     ## headline + supplementary decode throughput (bf16, fp8)
	$(PY) bench.py --gpus 1 --steps 3 --warmup 1 --full

bench-ds:       ## DisaggregatedSet lifecycle benchmark (config #4)
	$(PY) scripts/bench_ds.py --model llama-3-8b --steps 3 --warmup 1

smoke:
	$(PY) -c "import __graft_entry__ as g; g.build(); g.smoke()"

manager:        ## run the controller manager + API server
	$(PY) -m lws_amd --config examples/manager-config.yaml

plan-steps:     ## offline DS rollout previewer (hack/plan-steps analogue)
	$(PY) -m lws_amd.controllers.disaggregatedset.plan_steps \
	    --source '[2,6]' --target '[2,6]'

DOCKER ?= $(shell command -v docker || command -v podman || command -v buildah 2>/dev/null)
IMG_MANAGER ?= lws-amd-manager:latest
IMG_ENGINE ?= lws-amd-engine:latest

image:          ## build the controller-manager image (reference Dockerfile role)
	$(DOCKER) build -t $(IMG_MANAGER) -f Dockerfile .

image-engine:   ## build the MI355X engine image (vLLM-container analogue)
	$(DOCKER) build -t $(IMG_ENGINE) -f Dockerfile.engine .

crd-schemas:    ## regenerate declarative JSON Schemas (config/crd/bases analogue)
	$(PY) scripts/gen_crd_schema.py

clean:
	rm -rf lws_amd/ops/build lws_amd/ops/_C.so .pytest_cache
