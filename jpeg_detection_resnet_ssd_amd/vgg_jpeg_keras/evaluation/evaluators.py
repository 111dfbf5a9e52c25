"""The classifier's evaluator: same class name and method surface as classification_part/vgg_jpeg_keras/evaluation/
evaluators.py:6-66 (`Evaluator(generator=None)`, `__call__(model, test_generator=None)`, `make_runs`, `__str__`,
`display_results`, the `test_generator` property and the `score` attribute).  The score is whatever
`model.evaluate_generator` returns: [loss, top-1, top-5] for the classification configs."""
import numpy as np


class Evaluator(object):
    def __init__(self, generator=None):
        self.score = None
        self.runs = False
        self.number_of_runs = None
        self._generator = generator

    def _select_generator(self, test_generator):
        """A generator given with the call replaces the one given before; without either there is nothing to evaluate."""
        if test_generator is not None:
            self._generator = test_generator
        if self._generator is None:
            raise RuntimeError("A generator should be specified using the init or parameters.")
        return self._generator

    def __call__(self, model, test_generator=None):
        generator = self._select_generator(test_generator)
        self.runs = False
        self.score = model.evaluate_generator(generator, verbose=1)

    def make_runs(self, model, test_generator=None, number_of_runs=10):
        """`number_of_runs` passes over the generator; the score is their element-wise mean."""
        generator = self._select_generator(test_generator)
        self.runs = True
        scores = [model.evaluate_generator(generator) for _ in range(number_of_runs)]
        self.score = np.mean(np.array(scores), axis=0)
        self.number_of_runs = number_of_runs

    def __str__(self):
        if self.runs:
            return "Number of runs: {}\nAverage score: {}".format(self.number_of_runs, self.score)
        return "The evaluated score is {}.".format(self.score)

    @property
    def test_generator(self):
        return self._generator

    def display_results(self):
        print("The evaluated score is {}.".format(self.score))
