from magent_amd.builtin.rule_model import RandomActor, RunawayPrey, RushGatherer, RushPredator

__all__ = ["RandomActor", "RushPredator", "RunawayPrey", "RushGatherer"]
