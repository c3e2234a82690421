"""fastbn_amd -- MI355X-native FastBN hot paths (junction-tree inference, PC-stable CI sweep).

Python mirror of the reference's operator API over the C-ABI in ``include/fastbn.h``
(``libfastbn.so``, built in-tree by ``__graft_entry__.build()``).  The classes keep the
reference's names and argument meaning:

* ``JunctionTree(network, device).EvaluateAccuracy(...)`` / ``.infer(evidence)``
  -- ``JunctionTree`` + ``Inference`` (include/JunctionTree.h:19-94, include/Inference.h:23-49)
* ``PCStable(alpha, depth).StructLearnCompData(dataset, group_size)``
  -- include/PCStable.h:23-59
* ``IndependenceTest(dataset, alpha).IndependenceResult(x, y, z)``
  -- include/IndependenceTest.h:30-56
* ``ParameterLearning(source).LearnParamsKnowStructCompData(parents)``
  -- src/ParameterLearning.cpp:11-64 (``pdag_to_dag`` turns PC-stable's CPDAG into its input)
* ``LikelihoodWeighting(network, num_samples, seed, method="lw" | "pls").infer(evidence)``
  -- the reference's ``-a 5`` / ``-a 4`` stubs (src/main.cpp:97-121); ``Sampler(network).forward_sample(n, seed)``
  generates datasets on the device
* ``LoopyBeliefPropagation(network, iterations, tol, damping).infer(evidence)``
  -- the reference's ``-a 7`` stub (src/main.cpp:136-147); exact on polytrees, approximate on loopy graphs
* ``EPISBN(network, num_samples, iterations, tol, damping, eps, seed).infer(evidence)``
  -- the reference's ``-a 6`` stub (src/main.cpp:123-134): LBP's messages as the importance function of
  an unbiased sampler
* ``AISBN(network, num_samples, max_updates, interval, eps, seed).infer(evidence)`` and
  ``SelfImportanceSampling(...)`` -- the reference's ``-a 10`` / ``-a 8`` stubs (src/main.cpp:175-186,
  :149-160): samplers that learn their importance function from their own weighted samples
* ``MostProbableExplanation(network).infer(evidence)`` -- the complete assignment argmax_x P(x, e) and its
  log-probability, exact, by max-product on the junction forest (no reference counterpart)
* ``ExpectationMaximization(network).fit(data)`` -- the CPTs of a known structure from rows with missing
  cells (-1), by EM with exact junction-forest E-steps on the device (no reference counterpart)
* ``HillClimbing(score, max_parents, allowed, start).learn(source)`` -- score-based structure learning: greedy
  hill climbing under BIC / AIC / log-likelihood, family scores batched on the device and bit-identical to
  a host twin (no reference counterpart); ``family_scores(ci, families, penalty)`` scores arbitrary families

There is no CPU fallback: if the HIP library is missing, importing works but every call raises.
"""
from .api import (  # noqa: F401
    FastBNError,
    Network,
    Dataset,
    JunctionForest,
    JunctionTree,
    IndependenceTest,
    PCStable,
    PCResult,
    ParameterLearning,
    Sampler,
    LikelihoodWeighting,
    LoopyBeliefPropagation,
    EPISBN,
    AISBN,
    SelfImportanceSampling,
    MostProbableExplanation,
    ExpectationMaximization,
    HillClimbing,
    family_scores,
    hc_penalty,
    hc_table_bytes,
    score_marginals,
    family_sizes,
    pdag_to_dag,
    orient_skeleton,
    shd_bif,
    lib,
    load_libsvm,
    write_csv,
    write_libsvm,
    device_count,
    kernel_options,
)

__all__ = ["FastBNError", "Network", "Dataset", "JunctionTree", "JunctionForest", "IndependenceTest", "PCStable", "PCResult", "ParameterLearning",
           "Sampler", "LikelihoodWeighting", "LoopyBeliefPropagation", "EPISBN", "AISBN", "SelfImportanceSampling", "MostProbableExplanation", "ExpectationMaximization", "HillClimbing", "family_scores", "hc_penalty", "hc_table_bytes", "score_marginals",
           "family_sizes", "pdag_to_dag", "orient_skeleton", "shd_bif",
           "lib", "load_libsvm", "write_csv", "write_libsvm", "device_count", "kernel_options"]
