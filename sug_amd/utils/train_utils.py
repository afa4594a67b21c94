"""utils/train_utils.py: the class-balanced batch sampler the trainer hands to its loaders as `batch_sampler`."""
import random


class Sampler:
    """`classes`: per class the list of its sample indices (UnifiedPointDG.classes()).  An epoch picks class_per_batch
    classes once, then fills n_batches batches of batch_size samples: a class of the picked ones, then a sample of
    that class, both with random.choice -- the reference's sequence of draws, so random.seed(s) gives its batches."""

    def __init__(self, classes, class_per_batch, batch_size):
        self.classes = classes
        self.n_batches = sum(len(members) for members in classes) // batch_size
        self.class_per_batch = class_per_batch
        self.batch_size = batch_size

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        picked = random.sample(range(len(self.classes)), self.class_per_batch)
        batches = []
        for _ in range(self.n_batches):
            batch = []
            for _ in range(self.batch_size):
                klass = random.choice(picked)
                batch.append(random.choice(self.classes[klass]))
            batches.append(batch)
        return iter(batches)
